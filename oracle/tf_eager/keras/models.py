"""keras.models: a holder of what the functional graph would connect (the tensors are already computed)."""


class Model:
    def __init__(self, inputs=None, outputs=None, name=None):
        self.inputs, self.outputs, self.name = inputs, outputs, name
