"""Diagnostic: run bench.py's resnet workload against an alternative build of the library (tools only)."""
import sys, os, runpy
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azalea_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), sys.argv[1])
# an older build lacks the entry points added since (callers detect those by symbol: include/azx.h)
_lib.OPTIONAL.update(["azx_debug_stagger"])
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), run_name="__main__")
