"""Process-wide weights epoch.  A raw HIP kernel that rewrites parameters in place (FlatAdamW / FlatSGD / FlatRMSprop .step) does not
advance torch's per-tensor version counters, and neither does an in-place edit through `p.data`; caches of weight-derived tensors
(models.modules.layers.Derived) and captured forwards (mumpy_hip.graph.GraphedForward) therefore key on this epoch as well."""
weights_epoch = [0]

# a list while a GraphedForward warms up and captures: every Derived cache consulted is appended (models.modules.layers.Derived.get)
derived_seen = [None]


def bump_weights_epoch():
    """The one call to make after changing weights in a way torch cannot see: `p.data.mul_()`, `p.data.copy_()`, a kernel of your
    own writing into a parameter, or swapping an nn.Parameter object for another.  Every parameter-derived cache is rebuilt on its
    next use and every GraphedForward re-captures before its next replay; trainable and frozen parameters alike."""
    weights_epoch[0] += 1
