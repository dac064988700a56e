"""
Reference optima of the models of tests/cases_lm_scalars.py, solved in 400-bit arithmetic (mpmath; no other input), into
tests/golden/lm_scalars.npz: q* / scale and q* as float64 (hi, lo) pairs, the decisive Newton flag (-1: either value), and the digest
of the corpus they belong to.  tests/test_lm_scalars_host.py recomputes them and compares; tests/test_gpu_lm_scalars.py only reads them.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_lm_scalars.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_lm_scalars as K  # noqa: E402

if __name__ == "__main__":
    qrel, qstar, flag = K.compute_reference()
    np.savez_compressed(K.GOLDEN, qrel=qrel, qstar=qstar, flag=flag.astype(np.int8), digest=np.array(K.corpus_digest()))
    rows, fam = K.corpus()
    ok = K.checked(rows)
    print("{} rows, {} compared, Newton flag undecided on {}: {} bytes".format(len(rows), ok.sum(), (flag[ok] < 0).sum(), os.path.getsize(K.GOLDEN)))
