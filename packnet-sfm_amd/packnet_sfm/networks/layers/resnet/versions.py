"""The `version` string of DepthResNet / PoseResNet: '<layers>' or '<layers>pt' (ImageNet weights)."""
SUPPORTED = (18, 34)


def parse_version(version, what):
    """-> (number of layers, pretrained).  '50' (Bottleneck blocks) raises NotImplementedError naming it."""
    if version is None:
        raise AssertionError("%s needs a version" % what)
    digits, suffix = str(version)[:2], str(version)[2:]
    layers = int(digits)
    if layers == 50:
        raise NotImplementedError("%s version '50' (Bottleneck blocks) is not implemented on the gfx950 kernels: %s only"
                                  % (what, ' and '.join("'%d'" % n for n in SUPPORTED)))
    if layers not in SUPPORTED:
        raise AssertionError("ResNet version %s not available" % digits)
    return layers, suffix == 'pt'
