"""Small networks whose convolutions leave the one geometry the training tests used to see (one input feature, odd window,
'same', or stride 1): shared by tests/test_oracle_train.py, which checks the float64 oracle's gradients of these very networks
against finite differences on the CPU, and tests/test_gpu_train_conv.py, which checks the training step against that oracle.

Every builder takes a numpy RandomState and returns a layers.Serial that ends in a Softmax; nothing here touches the device."""
import numpy as np

STATES = 9


def _init(rs, scale=0.5):
    return lambda shape: (rs.normal(size=shape) * scale).astype(np.float32)


def first_layer(rs, winlen, stride, mode):
    """a. Convolution(1, 16, winlen, stride, mode, elu) -> Reverse(Gru) -> Gru"""
    from sloika_amd import activation, layers
    init = _init(rs)
    return layers.Serial([layers.Convolution(1, 16, winlen, stride, init=init, has_bias=True, fun=activation.elu, padding_mode=mode),
                          layers.Reverse(layers.Gru(16, 16, init=init, has_bias=True)),
                          layers.Gru(16, 16, init=init, has_bias=True),
                          layers.Softmax(16, STATES, init=init, has_bias=True)])


def multi_feature(rs, nfeat, winlen, stride, mode):
    """b. event-like input [T, B, nfeat]: a Convolution without bias over an Lstm"""
    from sloika_amd import layers
    init = _init(rs)
    return layers.Serial([layers.Convolution(nfeat, 16, winlen, stride, init=init, has_bias=False, padding_mode=mode),
                          layers.Lstm(16, 16, init=init, has_bias=True, has_peep=True),
                          layers.Softmax(16, 7, init=init, has_bias=True)])


def shrinks_twice(rs):
    """c. T shrinks at the first layer and again after a recurrent one: the gradients of the first two layers pass through
    the upper convolution's fold back onto its input at stride 3, 'same_left' at an even window"""
    from sloika_amd import activation, layers
    init = _init(rs)
    return layers.Serial([layers.Convolution(1, 8, 5, 2, init=init, has_bias=True, fun=activation.tanh),
                          layers.Reverse(layers.Gru(8, 16, init=init, has_bias=True)),
                          layers.Convolution(16, 12, 4, 3, init=init, has_bias=True, fun=activation.elu, padding_mode='same_left'),
                          layers.Gru(12, 16, init=init, has_bias=True),
                          layers.Softmax(16, 11, init=init, has_bias=True)])


def activations(rs, act, act2):
    """d. FeedForward(4, 6, tanh) -> Convolution(6, 8, 3, 2, act) -> Convolution(8, 8, 2, 1, 'valid', act2) -> Lstm(8, 16)"""
    from sloika_amd import activation, layers
    init = _init(rs)
    return layers.Serial([layers.FeedForward(4, 6, init=init, has_bias=True, fun=activation.tanh),
                          layers.Convolution(6, 8, 3, 2, init=init, has_bias=True, fun=getattr(activation, act)),
                          layers.Convolution(8, 8, 2, 1, init=init, has_bias=True, fun=getattr(activation, act2), padding_mode='valid'),
                          layers.Lstm(8, 16, init=init, has_bias=True, has_peep=True),
                          layers.Softmax(16, 7, init=init, has_bias=True)])


def parallel_branches(rs):
    """e. two Convolutions of different windows as the branches of a Parallel (both 'same': equal output lengths); the lower
    convolution's gradient is the sum of what the branches hand down"""
    from sloika_amd import activation, layers
    init = _init(rs)
    return layers.Serial([layers.Convolution(1, 8, 5, 2, init=init, has_bias=True),
                          layers.Parallel([layers.Convolution(8, 8, 3, 2, init=init, has_bias=True, fun=activation.tanh),
                                           layers.Convolution(8, 12, 7, 2, init=init, has_bias=True, fun=activation.elu)]),
                          layers.Gru(20, 16, init=init, has_bias=True),
                          layers.Softmax(16, 13, init=init, has_bias=True)])


def gru_on_convolution(rs, reverse):
    """f. a Gru directly above a Convolution of several input features: the Gru hands down dL/d(pre-activation) of the convolution,
    which folds it back onto the first convolution's output"""
    from sloika_amd import activation, layers
    init = _init(rs)
    gru = layers.Gru(16, 16, init=init, has_bias=True)
    return layers.Serial([layers.Convolution(1, 8, 5, 2, init=init, has_bias=True, fun=activation.elu),
                          layers.Convolution(8, 16, 3, 2, init=init, has_bias=True, fun=activation.tanh),
                          layers.Reverse(gru) if reverse else gru,
                          layers.Softmax(16, 17, init=init, has_bias=True)])


def spec_of(layer, dtype=None):
    """layer.spec() with the parameters a layer does not have set to None (the oracle returns gradients for the parameters
    that exist), its arrays cast to `dtype` if one is given."""
    from sloika_amd import layers
    if isinstance(layer, (layers.Serial, layers.Parallel)):
        return {"type": "serial" if isinstance(layer, layers.Serial) else "parallel",
                "sublayers": [spec_of(sub, dtype) for sub in layer.layers]}
    if isinstance(layer, layers.Reverse):
        return {"type": "reverse", "sublayer": spec_of(layer.layer, dtype)}
    spec = layer.spec()
    if not getattr(layer, "has_bias", True):
        spec["b"] = None
    if isinstance(layer, layers.Lstm) and not layer.has_peep:
        spec["p"] = None
    if dtype is not None:
        spec = {k: v.astype(dtype) if isinstance(v, np.ndarray) else v for k, v in spec.items()}
    return spec


def out_len(layer, T):
    """Output length of the network from its own layers (conv.py:66-77 for each Convolution on the way)."""
    from sloika_amd import layers
    if isinstance(layer, layers.Serial):
        for sub in layer.layers:
            T = out_len(sub, T)
        return T
    if isinstance(layer, layers.Parallel):
        lens = set(out_len(sub, T) for sub in layer.layers)
        assert len(lens) == 1, "branches of a Parallel disagree on the output length"
        return lens.pop()
    if isinstance(layer, layers.Reverse):
        return out_len(layer.layer, T)
    if isinstance(layer, layers.Convolution):
        return (T + layer.padding[0] + layer.padding[1] - layer.winlen) // layer.stride + 1
    return T


def batch(rs, net, T, B):
    """x:[T, B, insize], and labels and weights as long as the network's output."""
    x = rs.normal(size=(T, B, net.insize)).astype(np.float32)
    To = out_len(net, T)
    labels = rs.randint(0, net.size, size=(To, B)).astype(np.int32)
    weights = rs.uniform(0.5, 1.5, size=(To, B)).astype(np.float32)
    return x, labels, weights


def relu_margin(spec, tape):
    """Smallest |pre-activation| over the relu Convolution / FeedForward layers of an oracle_train tape (inf without one)."""
    t = spec["type"]
    if t == "serial":
        return min([relu_margin(s, tp) for s, tp in zip(spec["sublayers"], tape)] + [np.inf])
    if t == "reverse":
        return relu_margin(spec["sublayer"], tape)
    if t == "parallel":
        return min([relu_margin(s, tp) for s, tp in zip(spec["sublayers"], tape[0])] + [np.inf])
    if t in ("convolution", "feed-forward") and spec["activation"] == "relu":
        return float(np.abs(tape[1]).min())
    return np.inf


#: first-layer geometries (a): (winlen, stride, padding mode, T, B)
FIRST_LAYER = [(4, 1, 'same', 30, 3), (4, 1, 'same_left', 30, 2), (5, 3, 'valid', 61, 4), (5, 1, 'full', 25, 3),
               (11, 3, 'half', 70, 2), (16, 16, 'valid', 120, 3), (3, 5, 'valid', 64, 4), (6, 2, (1, 4), 41, 3),
               (11, 5, 'same', 9, 2)]
#: multi-feature first layers (b): (nfeat, winlen, stride, padding mode)
MULTI_FEATURE = [(nfeat, w, s, mode) for nfeat in (4, 12) for w, s, mode in ((5, 2, 'same'), (4, 3, 'same_left'))]
#: (d) (lower, upper) activations: each of the five that have a derivative kernel is once below and once above
ACT_PAIRS = [("tanh", "elu"), ("sigmoid", "tanh"), ("relu", "sigmoid"), ("elu", "linear"), ("linear", "relu")]


def _cases():
    """id -> (seed, T, B, builder(rs), (min_prob, l2, drop)); the loss settings go round the three of tests/test_gpu_train.py."""
    settings = [(0.0, 0.0, 0), (1e-3, 0.01, 1), (1e-30, 0.0, 0)]
    table = []
    for w, s, mode, T, B in FIRST_LAYER:
        name = mode if isinstance(mode, str) else "pad%d_%d" % mode
        table.append(("first-w%d-s%d-%s" % (w, s, name), T, B, lambda rs, w=w, s=s, mode=mode: first_layer(rs, w, s, mode)))
    for nfeat, w, s, mode in MULTI_FEATURE:
        table.append(("feat%d-w%d-s%d-%s" % (nfeat, w, s, mode), 37, 3,
                      lambda rs, nfeat=nfeat, w=w, s=s, mode=mode: multi_feature(rs, nfeat, w, s, mode)))
    table.append(("shrinks-twice", 83, 3, shrinks_twice))          # 83 -> 42 -> 14, the last two of the 42 under no window
    for act, act2 in ACT_PAIRS:
        table.append(("act-%s-%s" % (act, act2), 33, 2, lambda rs, act=act, act2=act2: activations(rs, act, act2)))
    table.append(("parallel-branches", 77, 3, parallel_branches))
    table.append(("gru-on-conv", 50, 4, lambda rs: gru_on_convolution(rs, False)))
    table.append(("reverse-gru-on-conv", 50, 4, lambda rs: gru_on_convolution(rs, True)))
    return {name: (RELU_SEEDS.get(name, 100 + k), T, B, build, settings[k % 3]) for k, (name, T, B, build) in enumerate(table)}


#: relu is discontinuous: seeds at which no pre-activation of a relu layer lies within 1e-4 of zero (the tests assert it), so
#: that a float32 sign flip cannot be blamed on a kernel
RELU_SEEDS = {"act-relu-sigmoid": 116, "act-linear-relu": 118}
CASES = _cases()
#: the cases whose oracle gradients tests/test_oracle_train.py checks against finite differences
FINITE_DIFFERENCE_CASES = (["first-w4-s1-same_left", "first-w5-s1-full", "first-w3-s5-valid", "first-w6-s2-pad1_4", "shrinks-twice"]
                           + ["act-%s-%s" % p for p in ACT_PAIRS] + ["parallel-branches", "gru-on-conv", "reverse-gru-on-conv"])


def make(name, dtype=None):
    """(net, spec, x, labels, weights, (min_prob, l2, drop)) of case `name`."""
    seed, T, B, build, settings = CASES[name]
    rs = np.random.RandomState(seed)
    net = build(rs)
    x, labels, weights = batch(rs, net, T, B)
    return net, spec_of(net, dtype), x, labels, weights, settings
