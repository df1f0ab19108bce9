"""keras.metrics: names only (the reference's loss modules import the package)."""


class Metric:
    def __init__(self, name=None, **kwargs):
        self.name = name
