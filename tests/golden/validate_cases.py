"""Cases of tests/golden/validate.npz (made by make_validate_goldens.py, which runs the reference's bin/validate_network.py:
wrap_network on them) and a float64 numpy restatement of what that function returns, shared by the generator and the tests.

A case is one of the small layer trees of layer_cases.py that end in a Softmax, an input recipe with a few hundred (t, b) rows, and
the seed its labels are drawn with.  Labels: about half the rows carry the arg-max of the reference's own float64 posterior, the rest
a uniform draw, so that the count of correct positions is neither 0 nor all."""
import numpy as np

import layer_cases as lc

#: a row is fragile when the float64 gap between its two largest posteriors is below this: twice the 1e-4 the project allows on
#: posteriors (design/scope.md a4, a6) -- only such a row's arg-max may legitimately differ on the device
FRAGILE_GAP = 2e-4
#: at most this share of a case's rows may be fragile (the generator asserts it for the reference's own output)
FRAGILE_SHARE = 0.01


def cases():
    """name -> {"tree", "x" (recipe [T, B, insize]), "label_seed"}.  Input seeds and scales are chosen so that the reference's own
    float64 posteriors have at most FRAGILE_SHARE fragile rows (these small random networks give flat posteriors, largest entry ~0.05
    over 65 states: of five seeds tried per case, 2 - 13 rows in ~300 were fragile)."""
    trees = lc.layer_cases()
    c = {}
    # a Gru stack behind a strided Convolution: 300 samples / stride 5 = 60 steps x 5 chunks = 300 rows, 65 states
    c["conv_rgr"] = {"tree": trees["serial_conv_rgr_softmax"]["tree"], "x": lc.recipe(910041, (300, 5, 1), 1.7), "label_seed": 1}
    # Window, birnn (Parallel of a Gru and a reversed Gru), FeedForward: 40 steps x 8 chunks = 320 rows, 65 states
    c["window_birnn"] = {"tree": trees["serial_window_birnn_ff_softmax"]["tree"], "x": lc.recipe(910032, (40, 8, 4), 2.0),
                         "label_seed": 2}
    # the output layer of the 5-mer models alone (96 -> 1025: the shape the split kernel takes): 20 x 12 = 240 rows
    c["softmax_1025"] = {"tree": lc.ser(trees["softmax_1025"]["tree"]), "x": lc.recipe(910003, (20, 12, 96), 4.0), "label_seed": 3}
    return c


def draw_labels(post, seed):
    """[T', B] int32 labels for a posterior [T', B, nstate]: the arg-max on about half of the rows, a uniform draw elsewhere."""
    rs = np.random.RandomState(seed)
    best = post.argmax(axis=2)
    rand = rs.randint(0, post.shape[2], size=best.shape)
    return np.where(rs.uniform(size=best.shape) < 0.5, best, rand).astype(np.int32)


def loss_rows(post, labels):
    """-log posterior[t, b, label] per position, float64 (T.nnet.categorical_crossentropy with integer targets)."""
    post = np.asarray(post, dtype=np.float64)
    return -np.log(np.take_along_axis(post, np.asarray(labels)[:, :, None].astype(np.int64), axis=2)[:, :, 0])


def correct_rows(post, labels):
    """1 where the first arg-max of the row is the label (T.eq(T.argmax(post, axis=2), labels)), int32."""
    return (np.asarray(post).argmax(axis=2) == np.asarray(labels)).astype(np.int32)


def loss_and_count(post, labels):
    """(mean row loss, number of correct positions) = what validate_network.py:46-54's `fv` returns."""
    return float(loss_rows(post, labels).mean()), int(correct_rows(post, labels).sum())


def top_two_gap(post):
    """Per row, the gap between the two largest posteriors (float64)."""
    top = np.sort(np.asarray(post, dtype=np.float64), axis=2)[:, :, -2:]
    return top[:, :, 1] - top[:, :, 0]
