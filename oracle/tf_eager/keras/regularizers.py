"""keras.regularizers: the object is carried, never applied (every shipped config has l2_reg 0)."""


class L2:
    def __init__(self, l2=0.01):
        self.l2 = float(l2)


def l2(l2=0.01):  # noqa: A001
    return L2(l2)
