"""GPU-only: record every GEMM-family launch (kernels.LAUNCHES) of one eager training step of each benchmark workload and write the
distinct launch descriptors, with the workloads that issue them and their count per step, as sorted JSON.

  python tools/trace_gemm_launches.py [out.json]          (default: tests/golden/gemm_launches.json)

tests/test_gemm_launches.py checks every descriptor at its real shape against float64 and that a fresh trace equals this fixture."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hcp_diffusion_amd import kernels as K  # noqa: E402
from workloads import BATCH, setup  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_launches.json")
KINDS = ("gemm", "gemm_lora", "gemm_geglu_bwd", "conv3x3", "wgrad_linear", "wgrad_conv3x3")     # the attention kinds: tools/trace_attention_launches.py


def trace_workload(workload, dev="cuda:0"):
    """{descriptor json: count} of one eager step (after a warm-up step that does the lazy packing; never a graph replay)."""
    tr, lat, ehs, kw = setup(workload, BATCH[workload], torch.device(dev))
    tr.train_one_step(lat, ehs, **kw)
    K.LAUNCHES = []
    try:
        tr.train_one_step(lat, ehs, **kw)
        torch.cuda.synchronize()
        launches = K.LAUNCHES
    finally:
        K.LAUNCHES = None
    counts = {}
    for d in launches:
        if d["kind"] not in KINDS:
            continue
        key = json.dumps(d, sort_keys=True)
        counts[key] = counts.get(key, 0) + 1
    del tr
    torch.cuda.empty_cache()
    return counts


def trace_all(workloads=("sd15", "dreambooth", "controlnet", "sdxl")):
    merged = {}
    for w in workloads:
        for key, n in trace_workload(w).items():
            merged.setdefault(key, {})[w] = n
    out = []
    for key in sorted(merged):
        out.append(dict(desc=json.loads(key), count=dict(sorted(merged[key].items()))))
    return out


def dumps(entries):
    """deterministic text: one descriptor per line."""
    lines = [json.dumps(e, sort_keys=True, separators=(",", ":")) for e in entries]
    return "[\n" + ",\n".join(lines) + "\n]\n"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    entries = trace_all()
    with open(path, "w") as f:
        f.write(dumps(entries))
    print(f"{len(entries)} distinct launch descriptors -> {path}")


if __name__ == "__main__":
    main()
