"""bench.py on a library variant built from an older commit.  Where that library has no addend entries
(jd_npred_poisson_batch_addends_fwd_bwd, jd_adam_step_addends): the binding loads strictly, so the two entries are taken out
of it for this process, and the session never offers addend images -- the joint step then is the older library's own.  A
library that has them runs unchanged.  For A/B runs against a parent build:

    JOLIDECO_HIP_LIBRARY=jolideco_amd/libjolideco_hip_parent.so python tools/bench_old_library.py --config c3 --repeats 9

(tools/ab_bench_libs.sh alternates it with the in-tree build.)"""
import ctypes
import os
import runpy
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from jolideco_amd import _hip, core  # noqa: E402

_path = os.environ.get("JOLIDECO_HIP_LIBRARY")
if not _path:
    sys.exit("tools/bench_old_library.py: set JOLIDECO_HIP_LIBRARY to the library variant to run (see the docstring)")
_lib = ctypes.CDLL(os.path.abspath(_path))
_missing = [name for name in ("jd_npred_poisson_batch_addends_fwd_bwd", "jd_adam_step_addends") if not hasattr(_lib, name)]
for name in _missing:  # (a parent that has the entries runs as it is: the wrapper then is plain bench.py on that library)
    _hip.EXPORTS.pop(name)
if _missing:
    core.FitSession._likelihood_addends = lambda self, early: None
for name in ("jd_conv_plan_direct_kernel", "jd_conv_plan_fft_route"):  # queries that only tests ask: a library without them runs the same steps
    if not hasattr(_lib, name):
        _hip.EXPORTS.pop(name)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
