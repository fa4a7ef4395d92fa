"""Records pipeline.prescribe's default call (planner="sweep") on the synthetic tracker file of examples/prescribe_from_csv.py
into tests/golden/prescribe_sweep_default.npz (needs a GPU): the list of keys and the arrays tests/test_npi_plan_pipeline.py
compares bit for bit.  Run from the repository root:  python tests/golden/make_golden_prescribe_sweep.py [out.npz]"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from epidemicmodeling_amd import pipeline  # noqa: E402
from tests import test_npi_plan_pipeline as T  # noqa: E402

if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    cases, deaths, N, ip = T.synthetic_inputs(tempfile.mkdtemp())
    out = pipeline.prescribe(cases, deaths, N, ip, horizon=T.HORIZON, n_eps=T.N_EPS)
    np.savez_compressed(dst, keys=np.array(list(out)), **{k: np.asarray(out[k]) for k in T.RECORDED})
    print(dst, list(out))
