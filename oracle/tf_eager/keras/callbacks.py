"""keras.callbacks: the base-class name the reference's modules import."""


class Callback:
    def __init__(self, **kwargs):
        self.model = None
