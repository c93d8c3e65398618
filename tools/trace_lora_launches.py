"""GPU-only: record every grouped LoRA weight-gradient launch (kernels.LAUNCHES, kind lora_wgrad_grouped) of one eager training step of
the sd15 and sdxl workloads and write, as sorted JSON, the distinct per-layer geometries (M, K, N, r, slot0, splits, leading dimensions,
residual-half offsets, the target the call settled on; not the scale, a learned or derived float that selects no code path) with their count per workload, and each grouped call's composition as
indices into them.

  python tools/trace_lora_launches.py [out.json]          (default: tests/golden/lora_launches.json)

tests/test_lora_launches.py checks every geometry and each workload's whole call at the real shapes against float64 and that a fresh
trace equals this fixture."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hcp_diffusion_amd import kernels as K  # noqa: E402
from workloads import BATCH, setup  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lora_launches.json")
KINDS = ("lora_wgrad", "lora_wgrad_pair", "lora_wgrad_grouped")


def trace_workload(workload, dev="cuda:0"):
    """the lora_wgrad* records of one eager step (after a warm-up step; never a graph replay)."""
    tr, lat, ehs, kw = setup(workload, BATCH[workload], torch.device(dev))
    tr.train_one_step(lat, ehs, **kw)
    K.LAUNCHES = []
    try:
        tr.train_one_step(lat, ehs, **kw)
        torch.cuda.synchronize()
        launches = [d for d in K.LAUNCHES if d["kind"] in KINDS]
    finally:
        K.LAUNCHES = None
    del tr
    torch.cuda.empty_cache()
    return launches


def trace_all(workloads=("sd15", "sdxl")):
    geos, calls = {}, {}
    for w in workloads:
        calls[w] = []
        for rec in trace_workload(w):
            assert rec["kind"] == "lora_wgrad_grouped", f"{w} launches {rec['kind']}: this fixture holds grouped calls only"
            keys = [json.dumps(dict({k: v for k, v in l.items() if k != "scale"}, target=rec["target"]), sort_keys=True) for l in rec["layers"]]
            for k in keys:
                geos.setdefault(k, {}).setdefault(w, 0)
                geos[k][w] += 1
            calls[w].append((rec["target"], keys))
    order = {k: i for i, k in enumerate(sorted(geos))}
    return dict(geometries=[dict(geo=json.loads(k), count=dict(sorted(geos[k].items()))) for k in sorted(geos)],
                calls={w: [dict(target=t, layers=[order[k] for k in keys]) for t, keys in cs] for w, cs in sorted(calls.items())})


def dumps(fx):
    """deterministic text: one geometry, one call per line."""
    js = lambda e: json.dumps(e, sort_keys=True, separators=(",", ":"))
    geo = ",\n".join(js(e) for e in fx["geometries"])
    calls = ",\n".join(f'{js(w)}:[\n' + ",\n".join(js(c) for c in cs) + "\n]" for w, cs in sorted(fx["calls"].items()))
    return '{"calls":{\n' + calls + '\n},\n"geometries":[\n' + geo + "\n]}\n"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    fx = trace_all()
    with open(path, "w") as f:
        f.write(dumps(fx))
    print(f"{len(fx['geometries'])} distinct layer geometries, {sum(len(c) for c in fx['calls'].values())} grouped calls -> {path}")


if __name__ == "__main__":
    main()
