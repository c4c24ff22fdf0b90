"""Inputs shared by tests/test_lr_l1_cpu.py, tests/test_lr_l1_gpu.py, tests/test_lr_l1_fenced_gpu.py and tests/golden/make_lr_l1_golden.py:
the banks and row lists of tests/logreg_cases.py under the strengths the L1 tests use (no case is standardised: there is no scaled L1
classifier).

CASES: name -> C (None = the case's own C per problem).  case(name) -> the logreg case with C replaced; problems(c) and x_hash(c) are
those of logreg_cases."""
import numpy as np

import logreg_cases
from logreg_cases import problems, x_hash  # noqa: F401

CASES = {
    "n10_k2_dim1024": 1.0,                 # K = 2: the mirror
    "n7_k3_dim37": 10.0,                   # dim is no multiple of the wave
    "ragged_50_20_64": 1.0,                # lists that start inside the flat list, shared and repeated rows, poisoned bank rows nobody names
    "65_problems_of_8_dim16": 30.0,        # 195 workgroups
    "k6_n200_raw": 1.0,                    # the harness shape
    "c_0p01_1_100": None,                  # per-problem C: 0.01, 1, 100
    "absent_class": 10.0,                  # a class with no sample
    "constant_column_scaled": 10.0,        # (unscaled here) a constant and a zero column
    "caps_n1024_k8_dim1024": None,         # the caps; its own C = 0.05
}
AGAINST_SKLEARN = ["k6_n200_raw", "absent_class", "constant_column_scaled"]      # where the device is held to sklearn's default run

_CACHE = {}


def case(name):
    if name not in _CACHE:
        c = dict(logreg_cases.case(name))
        if CASES[name] is not None:
            c["C"] = np.full(len(c["offsets"]) - 1, CASES[name], np.float64)
            c["C"].setflags(write=False)
        c["standardize"] = False
        _CACHE[name] = c
    return _CACHE[name]


def golden_key(name, what):
    return f"{name}/{what}"


def dense_star(g, name, P, K, dim):
    """The optimum's (coef float64 [P, K, dim], intercept [P, K]) from the sparse triplets of the golden file."""
    W = np.zeros((P, K, dim + 1))
    at = g[golden_key(name, "w_index")].astype(np.int64)
    W.reshape(-1)[at] = g[golden_key(name, "w_value")]
    return W[:, :, :dim], W[:, :, dim]
