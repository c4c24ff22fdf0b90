"""Generates tests/golden/svc_proba_golden.npz on the CPU (sklearn is needed here and only here): for every case of
tests/svc_proba_cases.py the arrays of svc_proba_cases.reference (its docstring names them), under the key "<case>/<array>", plus
"<case>/x_sha1", a hash of the bank.

Asserted here, so that the tests may rely on it: at least 90 % of every problem's evaluation rows have a top-two gap in p_star above
2 e_p, and the case made for them meets each of the three rules for a sub-fit that lacks a class.

The GPU tests read only this file plus NumPy."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from svc_cases import x_hash  # noqa: E402
from svc_proba_cases import CASES, case, reference  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in CASES:
        t0 = time.time()
        ref = reference(name, log=print)
        print(f"{name}: e_cv {ref['e_cv'].max():.2e} e_p {ref['e_p'].max():.2e} clear {ref['clear'].min():.2f} rules {ref['rules'].tolist()} "
              f"({time.time() - t0:.1f} s)")
        assert ref["clear"].min() >= 0.9, (name, ref["clear"])
        if name == "degenerate_1_2_1_10":
            assert (ref["rules"] > 0).all(), ref["rules"]
        for key, value in ref.items():
            out[f"{name}/{key}"] = value
        out[f"{name}/x_sha1"] = np.asarray(x_hash(case(name)))
    path = os.path.join(HERE, "svc_proba_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
