"""An independent numpy restatement of Optimizer::BundleAdjustment (src/Optimizer.cc:49-237 on g2o) for the tests of
orbp_bundle_adjustment / orbm_bundle_adjustment.  The graph, the Schur complement and the Levenberg loop are those of
tests/lba_oracle.py (rotation matrices, chain-rule Jacobians, a dense Schur product, LAPACK: not the product's text); what is
BundleAdjustment's own is stated here: one optimize(n_iterations), Huber with sqrt(5.99) / sqrt(7.815) held as floats (:85-86;
LocalBundleAdjustment has 5.991) or no kernel at all, no flagging pass, and every local key frame written back.

tests/lba_oracle.py is not edited: this module loads a private second instance of it and sets that instance's Huber deltas.

order = "forward" / "reverse" as there.  Returns a dict: Tcw float64 [n_local, 4, 4], xw float64 [n_points, 3], stats (iterations,
trials, lambda, chi2), margin = the smallest relative distance of any decision (rho against 0 in every trial, which decides accept /
reject, the trial loop's end and the rho == 0 termination; (iniChi - currentChi) * 1e3 against iniChi, which feeds _nBad) from its
boundary, transcript = [(0, iteration, trial, accepted)], ended_by_nbad."""
import importlib.util
import math
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_lba_oracle_for_ba", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lba_oracle.py"))
lo = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lo)
lo.DELTA_MONO = float(np.float32(math.sqrt(5.99)))
lo.DELTA_STEREO = float(np.float32(math.sqrt(7.815)))


def bundle_adjustment(pr, n_iterations=5, robust=True, order="forward"):
    g = lo.Graph(pr, order)
    g.robust = bool(robust)
    stats = {"iterations": [0, 0], "trials": [0, 0], "lambda": 0.0, "chi2": 0.0}
    g.optimize(0, n_iterations, stats)
    Tcw = np.zeros((g.n_local, 4, 4))
    for k in range(g.n_local):
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = g.R[k], g.t[k], 1.0
    it, tr = stats["iterations"][0], stats["trials"][0]
    last = [t for t in g.transcript if t[1] == it - 1]
    # the loop ended before its budget, and neither by ten trials nor by rho == 0: the _nBad counter ended it
    ended_by_nbad = 0 < it < n_iterations and len(last) < 10 and last[-1][3]
    return {"Tcw": Tcw, "xw": g.X.copy(), "stats": {"iterations": it, "trials": tr, "lambda": stats["lambda"], "chi2": stats["chi2"]},
            "margin": g.margin, "transcript": g.transcript, "ended_by_nbad": bool(ended_by_nbad)}
