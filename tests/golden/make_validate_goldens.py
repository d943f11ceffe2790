#!/usr/bin/env python3
"""Golden vectors for sloika_amd.validate, produced by executing the reference's own `bin/validate_network.py:wrap_network`
UNMODIFIED on the cases of validate_cases.py, under tests/golden/theano_standin (see make_layer_goldens.py) in float64.

    python tests/golden/make_validate_goldens.py          # -> tests/golden/validate.npz, tests/golden/validate_cases.json

Per case: the labels, the loss and the count `fv(x, labels)` returned, and per (t, b) row the float64 loss term, the correct flag and
the gap between the two largest posteriors (from the reference network's own compiled forward pass).  Inputs and weights are
recipes.  Only data is written: no reference source is stored.
"""
import importlib.util
import json
import os
import sys
import warnings

os.environ.setdefault("THEANO_STANDIN_FLOATX", "float64")
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import layer_cases as lc  # noqa: E402
import make_layer_goldens as mlg  # noqa: E402
import validate_cases as vc  # noqa: E402


def load_validate_network_module():
    path = os.path.join(mlg.REF, "bin", "validate_network.py")
    spec = importlib.util.spec_from_file_location("ref_validate_network", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)                                    # argparse set-up only; __main__ block not run
    return mod


def main():
    mlg.setup_reference()
    assert mlg.floatx() == np.float64
    vn = load_validate_network_module()
    arrays, meta = {}, {}
    for name, c in vc.cases().items():
        net = mlg.build_reference(c["tree"])                            # (records conv.calculate_padding's answer in the tree)
        x = lc.expand(c["x"], np.float64)
        post = np.asarray(net.compile()(x), dtype=np.float64)
        labels = vc.draw_labels(post, c["label_seed"])
        loss, ncorrect = vn.wrap_network(net)(x, labels)
        loss, ncorrect = float(loss), int(ncorrect)
        gap = vc.top_two_gap(post)
        nfragile = int((gap < vc.FRAGILE_GAP).sum())
        assert nfragile <= vc.FRAGILE_SHARE * gap.size, (name, nfragile, gap.size)
        want_loss, want_count = vc.loss_and_count(post, labels)
        assert ncorrect == want_count and abs(loss - want_loss) <= 1e-12 * abs(want_loss), (name, loss, want_loss, ncorrect, want_count)
        arrays[name + "/labels"] = labels
        arrays[name + "/loss_rows"] = vc.loss_rows(post, labels)
        arrays[name + "/correct_rows"] = vc.correct_rows(post, labels)
        arrays[name + "/gap"] = gap
        meta[name] = {"tree": c["tree"], "x": c["x"], "label_seed": c["label_seed"], "loss": loss, "ncorrect": ncorrect,
                      "rows": int(gap.size), "fragile_rows": nfragile, "sha256": mlg.input_sha(c["tree"], c["x"])}
        print("%-14s rows %4d  loss %.9f  ncorrect %4d  fragile %d  smallest gap %.3g" % (name, gap.size, loss, ncorrect, nfragile, gap.min()))
    np.savez_compressed(os.path.join(HERE, "validate.npz"), **arrays)
    with open(os.path.join(HERE, "validate_cases.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    for f in ("validate.npz", "validate_cases.json"):
        print("%-24s %9d bytes" % (f, os.path.getsize(os.path.join(HERE, f))))


if __name__ == "__main__":
    main()
