"""Writes tests/golden/pt_reference.pt: what the reference's OWN EmbeddingPTHook (hcpdiff/models/text_emb_ex.py) produces when hooked
onto the oracle CLIP text model — the conditioning states and the embedding rows (hook output + position embedding, fp32) for a small
model with two custom words (4 and 2 vectors) and tokenizer_repeats = 2.  Run where the reference tree exists; the GPU suite then pins
the native path against the recorded numbers (tests/test_prompt_tuning.py::test_encoder_matches_the_reference_hook_fixture).

    python tools/gen_pt_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from oracle.clip_ref import OracleCLIPTextModel
    from oracle.unet_sd15 import seeded_init_
    from pt_ref import StubTokenizer
    from test_prompt_tuning import _HFish, _load_reference_pt_hook
    RefHook, _ = _load_reference_pt_hook()
    cfg = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77)
    ora = seeded_init_(OracleCLIPTextModel(**cfg), 31).eval()
    g = torch.Generator().manual_seed(32)
    words = {"pt-four": torch.randn(4, 64, generator=g) * 0.5, "pt-two": torch.randn(2, 64, generator=g) * 0.5}
    tk = StubTokenizer(100)
    RefHook.hook({w: torch.nn.Parameter(v.clone(), requires_grad=False) for w, v in words.items()}, tk, _HFish(ora), N_repeats=2)
    ids = torch.randint(0, 98, (3, 154), generator=g); ids[:, 0] = 98
    a, b = tk.added["pt-four"], tk.added["pt-two"]
    ids[0, 5] = a; ids[0, 6] = b; ids[1, 74] = a; ids[1, 76] = b; ids[1, 140] = a; ids[2, 150] = b; ids[2, 151] = a
    with torch.no_grad():
        states = ora.encode(ids, n_repeats=2)
        e = ora.text_model.embeddings
        embeddings = e.token_embedding(ids.reshape(6, 77)) + e.position_embedding(torch.arange(77)[None])
    out = dict(config=cfg, n_repeats=2, state={k: v.clone() for k, v in ora.state_dict().items()}, words=words, ids=ids,
               states=states, embeddings=embeddings)
    path = os.path.join(ROOT, "tests", "golden", "pt_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
