"""python tools/bench_with_lib.py <libclx.so> [--script tools/bench_X.py] [the script's arguments]: bench.py, or the
script named, on a library built from another checkout, to compare it with this one's."""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellulus_amd import _clx
_clx.LIB_PATH = os.path.abspath(sys.argv[1])
rest = sys.argv[2:]
script = os.path.join(ROOT, "bench.py")
if rest[:1] == ["--script"]:
    script, rest = os.path.abspath(rest[1]), rest[2:]
    sys.path.insert(0, os.path.dirname(script))
sys.argv = [os.path.basename(script)] + rest
runpy.run_path(script, run_name="__main__")
