"""rocprofv3 --pmc target (tools/pmc_msda_run.sh): the MSDA forward at BASELINE cfg 4, B = 8, three launches per route.
MSDA_ROUTES: comma-separated of general (generation 4 through the general-geometry hint), auto (generation 9), gather."""
import sys, os, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench
from bench_msda import forward_general, set_tiled
from visionllm_amd import ms_deform_attn as A
dev = "cuda:0"
t = bench.build_msda_inputs(dev, 8, 200)["enc"]
run = lambda: A.ms_deform_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["attw"], 64)
routes = {"general": (1, lambda: forward_general(t)), "auto": (1, run), "gather": (0, run)}
for r in os.environ.get("MSDA_ROUTES", "general,auto").split(","):
    tiled, fn = routes[r]
    set_tiled(tiled)
    for _ in range(3):
        fn()
torch.cuda.synchronize()
