"""keras.initializers: only Constant initialises anything (oracle/tf_eager/keras/layers.py: add_weight)."""


class Constant:
    def __init__(self, value=0):
        self.value = value
