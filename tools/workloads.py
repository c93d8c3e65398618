"""The benchmark workloads of BASELINE.json as one eager training step each: shared set-up of tools/autotune.py (tuning sweeps) and
tools/trace_gemm_launches.py (the launch fixture of tests/test_gemm_launches.py).  Importing this module binds no kernel library."""
import torch

from hcp_diffusion_amd.trainer import NativeTrainer
from hcp_diffusion_amd.unet import SDXL_CONFIG, NativeUNet2DConditionModel

BF = torch.bfloat16
PATS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]
# workload -> default batch: SD1.5 LoRA r8, DreamBooth full fine-tune, ControlNet, SDXL LoRA r16 at 1024 px
BATCH = {"sd15": 4, "dreambooth": 2, "controlnet": 4, "sdxl": 2}


def setup(workload, B, dev):
    """(trainer, latents, text states, extra step kwargs) of one workload, weights seeded on the device."""
    sdxl = workload == "sdxl"
    with torch.device("meta"):
        unet = NativeUNet2DConditionModel(**SDXL_CONFIG) if sdxl else NativeUNet2DConditionModel()
    unet = unet.to_empty(device=dev)
    with torch.no_grad():
        for n, p in unet.named_parameters():
            p.normal_(0, 0.02) if p.dim() > 1 else p.fill_(1.0 if n.endswith("weight") else 0.0)
    kw = {}
    if workload == "dreambooth":
        tr = NativeTrainer(unet, None, train_cfg=[dict(layers=[""], lr=1e-6)])
    elif workload == "controlnet":
        from hcp_diffusion_amd.controlnet import make_controlnet
        plug = make_controlnet(unet)
        with torch.no_grad():
            for m in list(plug.controlnet_down_blocks) + [plug.controlnet_mid_block, plug.cond_head[-1]]:
                m.weight.normal_(0, 0.02)
        tr = NativeTrainer(unet, None, plugins=[(plug, 1e-4)])
        kw["plugin_input"] = dict(cond=torch.rand(B, 3, 512, 512, device=dev))
    else:
        tr = NativeTrainer(unet, [dict(layers=PATS, rank=16 if sdxl else 8)])
        with torch.no_grad():
            for blk in tr.bucket.blocks:
                blk.layer.W_up.normal_(0, 0.02)
        tr.bucket.pack()
    hw, cd = (128, 2048) if sdxl else (64, 768)
    lat = torch.randn(B, 4, hw, hw, device=dev); ehs = torch.randn(B, 77, cd, device=dev).to(BF)
    if sdxl:
        kw["added_cond_kwargs"] = dict(text_embeds=torch.randn(B, 1280, device=dev), time_ids=torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B, device=dev))
    return tr, lat, ehs, kw
