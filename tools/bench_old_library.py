"""bench.py on a library variant built from a commit that has no addend entries (jd_npred_poisson_batch_addends_fwd_bwd,
jd_adam_step_addends): the binding loads strictly, so the two entries are taken out of it for this process, and the session
never offers addend images -- the joint step then is the older library's own.  For A/B runs against a parent build:

    JOLIDECO_HIP_LIBRARY=jolideco_amd/libjolideco_hip_parent.so python tools/bench_old_library.py --config c3 --repeats 9

(tools/ab_bench_libs.sh alternates it with the in-tree build.)"""
import os
import runpy
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from jolideco_amd import _hip, core  # noqa: E402

for name in ("jd_npred_poisson_batch_addends_fwd_bwd", "jd_adam_step_addends"):
    _hip.EXPORTS.pop(name)
core.FitSession._likelihood_addends = lambda self, early: None
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
