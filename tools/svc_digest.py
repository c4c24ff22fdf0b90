"""What the support-vector fits write, as one SHA-256 per call: two builds of the library that print the same listing compute the same
bytes.  For every case of tests/svc_cases.py one svc.fit_on_device call, for every case of tests/svc_proba_cases.py one
svc.fit_proba_on_device call under the case's folds, each at the tests' settings (tol 1e-5, max_iter 100000, platt_eps 1e-8) and again
with max_iter = 3, where every pair is cut mid-flight and the state after exactly three steps is what is hashed.  The digest covers
coef, rho, gamma, centre, inv_scale, info, gap, and for the proba calls probA, probB, cv_decision, cv_info, present, in that order.
Needs a GPU, neither sklearn nor a fixture.  MKWS_LIB selects the build (multilingual_kws_amd/_lib.py):

  python tools/svc_digest.py > new.txt;  MKWS_LIB=/path/to/other/libmkws_hip.so python tools/svc_digest.py > other.txt;  diff new.txt other.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import svc_cases  # noqa: E402
import svc_proba_cases  # noqa: E402

from multilingual_kws_amd import svc  # noqa: E402

FIT = ("coef", "rho", "gamma", "centre", "inv_scale", "info", "gap")
PROBA = FIT + ("probA", "probB", "cv_decision", "cv_info", "present")


def digest(fit, fields):
    h = hashlib.sha256()
    for name in fields:
        h.update(getattr(fit, name).tobytes())
    return h.hexdigest()


def main():
    for max_iter in (100000, 3):
        for name in svc_cases.CASES:
            c = svc_cases.case(name)
            fit = svc.fit_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], C=c["C"], standardize=c["standardize"], tol=1e-5,
                                    max_iter=max_iter)
            print(f"fit        {name:<28} max_iter {max_iter:<6} {digest(fit, FIT)}", flush=True)
        for name in svc_proba_cases.CASES:
            c = svc_proba_cases.case(name)
            fit = svc.fit_proba_on_device(c["x"], c["rows"], c["labels"], c["offsets"], c["n_classes"], folds=c["folds"], n_folds=c["n_folds"], C=c["C"],
                                          standardize=c["standardize"], tol=1e-5, max_iter=max_iter, platt_eps=1e-8)
            print(f"fit_proba  {name:<28} max_iter {max_iter:<6} {digest(fit, PROBA)}", flush=True)


if __name__ == "__main__":
    main()
