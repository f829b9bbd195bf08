"""Record the reference's adaptive loss weights (pinnrl/components/adaptive_weights.py) on fixed input sequences.

    python tools/make_adaptive_golden.py --reference /path/to/the/reference/checkout

Runs only where the reference package is present.  Writes tests/golden/adaptive_weights.npz (arrays only, a few KB):

    values            (2, 6, 3) fp32   two sequences of 6 calls x 3 positive values, magnitudes spread over 1e-4 .. 1e2
    alpha, eps        (3,)      fp64   the three settings
    initial_weights   (3, 3)    fp32   per setting; a row of NaN = no initial weights
    weights           (2 strategies [rbw, lrw], 3 settings, 2 sequences, 6 calls, 3) fp32: what `update` returned

tests/test_adaptive_weights_cpu.py holds the fp64 restatement (tests/adaptive_model.py) and the product's `_EmaLossWeights`
against these numbers.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRATEGIES = ("rbw", "lrw")
SETTINGS = ((0.9, 1e-5, [0.5, 0.3, 0.2]), (0.7, 1e-6, [0.3, 0.4, 0.3]), (0.9, 1e-5, None))


def sequences():
    rng = np.random.default_rng(20240611)
    # log-uniform over 1e-4 .. 1e2, the three components on different scales and moving from call to call
    return (10.0 ** rng.uniform(-4.0, 2.0, size=(2, 6, 3))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PINNRL_REFERENCE"), help="checkout that holds the pinnrl package")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "adaptive_weights.npz"))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "pinnrl")):
        sys.exit("the reference package is not here: pass --reference (or set PINNRL_REFERENCE)")
    sys.path.insert(0, args.reference)
    from pinnrl.components.adaptive_weights import AdaptiveLossWeights  # noqa: E402  (reference)

    values = sequences()
    weights = np.zeros((len(STRATEGIES), len(SETTINGS), values.shape[0], values.shape[1], 3), dtype=np.float32)
    for si, strategy in enumerate(STRATEGIES):
        for ci, (alpha, eps, init) in enumerate(SETTINGS):
            for qi in range(values.shape[0]):
                rule = AdaptiveLossWeights(strategy=strategy, alpha=alpha, eps=eps, initial_weights=init)
                for k in range(values.shape[1]):
                    v = torch.from_numpy(values[qi, k].copy())
                    w = rule.update(losses=v) if strategy == "rbw" else rule.update(gradients=v)
                    weights[si, ci, qi, k] = w.detach().numpy()
    init = np.array([i if i is not None else [np.nan] * 3 for _, _, i in SETTINGS], dtype=np.float32)
    np.savez(args.out, values=values, alpha=np.array([s[0] for s in SETTINGS]), eps=np.array([s[1] for s in SETTINGS]),
             initial_weights=init, weights=weights)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
