"""Diagnostic: run a tools/ script against an alternative build of the library: python tools/lib_run.py <lib.so> <script.py> [args]"""
import os, runpy, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azalea_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), sys.argv[1])
# an older build lacks the entry points added since (callers detect those by symbol: include/azx.h)
_lib.OPTIONAL.update(["azx_match_set_harvest", "azx_match_set_first_mover", "azx_match_rows", "azx_tournament_set_harvest",
                      "azx_tournament_set_first_mover", "azx_tournament_rows", "azx_rows_read"])
script = sys.argv[2]
sys.argv = [script] + sys.argv[3:]
runpy.run_path(script, run_name="__main__")
