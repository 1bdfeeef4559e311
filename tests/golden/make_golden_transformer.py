"""Generates tests/golden/transformer.npz FROM THE REFERENCE'S OWN SimpleTransformer.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_transformer.py
The reference is imported unmodified through oracle/ref_shim.py; what is committed are inputs and expected outputs only.  Parameters
come from the deterministic recipe in oracle/weights.py (the positional-encoding buffer ``pe.pe`` keeps the reference's own table), so
the tests rebuild the same networks without committed weights.  Every case runs the reference's GenerateLoopV2 on CPU; the MLP head's
raw outputs are captured at every step with a forward hook.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_shim import load_reference  # noqa: E402
from oracle.weights import recipe_state_dict  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ref = load_reference()
tr = importlib.import_module("mimikit.networks.transformers")
torch.set_grad_enabled(False)

# tag: (network keywords, IO keywords, clips, prompt length, steps, recipe seed)   (tests/test_gpu_transformer.py: CASES)
CASES = {
    "mlp0": (dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=16), dict(kind="mulaw", n_mlp_layers=0), 3, 20, 24, 61),
    "mlp2_ln": (dict(model_dim=64, n_heads=8, feedforward_dim=128, num_layers=2, rf=16, with_layer_norm=True),
                dict(kind="mulaw", n_mlp_layers=2), 3, 20, 24, 62),
    "rf1": (dict(model_dim=32, n_heads=4, feedforward_dim=64, num_layers=1, rf=1), dict(kind="mulaw", n_mlp_layers=1), 3, 4, 16, 63),
    "magspec": (dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=8, with_layer_norm=True), dict(kind="magspec", n_fft=64),
                3, 10, 12, 64),
}
MIN_GAP = 1e-3
GAIN = 1.5


def io_spec(io_kw):
    if io_kw["kind"] == "mulaw":
        return ref.IOSpec.mulaw_io(ref.IOSpec.MuLawIOConfig(input_module_type="embedding", mlp_dim=32, n_mlp_layers=io_kw["n_mlp_layers"]))
    return ref.IOSpec.magspec_io(ref.IOSpec.MagSpecIOConfig(n_fft=io_kw["n_fft"], hop_length=io_kw["n_fft"] // 4))


def fill(net, seed):
    """the recipe for every parameter; the positional-encoding buffer stays the reference's table"""
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if torch.is_floating_point(v) and v.dim() > 0 and k != "pe.pe"}
    for k, v in recipe_state_dict(shapes, seed, GAIN).items():
        sd[k].copy_(v)


def run_loop(net, prompts, n_steps):
    cfg = ref.GenerateLoopV2.Config(parameters=None, yield_inversed_outputs=False, display_waveform=False, write_waveform=False)
    loop = ref.GenerateLoopV2(cfg, net, n_steps, dataloader=[[np.arange(prompts[0].size(0)), *prompts]], logger=None)
    outs = [o for o in loop.run()]
    torch.set_grad_enabled(False)   # the reference loop re-enables grad globally in teardown
    return outs[0]


def make():
    g = torch.Generator().manual_seed(2024)
    arrays = {}
    for tag, (net_kw, io_kw, clips, prompt_len, n_steps, seed) in CASES.items():
        net = tr.SimpleTransformer.from_config(tr.SimpleTransformer.Config(io_spec=io_spec(io_kw), **net_kw)).eval()
        fill(net, seed)
        if io_kw["kind"] == "mulaw":
            prompt = torch.randint(0, 256, (clips, prompt_len), generator=g)
            log = []
            h = net.output_modules[0].estimator[0].fc.register_forward_hook(lambda m, i, o: log.append(o.detach().clone()))
            out = run_loop(net, (prompt,), n_steps)[0]
            h.remove()
            raw = torch.cat(log, 1)                                    # (clips, n_steps, 256 + 1)
            top = torch.topk(raw[..., :-1], 2, dim=-1).values
            gap = float((top[..., 0] - top[..., 1]).min())
            assert gap >= MIN_GAP, f"{tag}: smallest top-2 logit gap {gap:.2e} < {MIN_GAP}: pick another seed"
            arrays.update({f"{tag}_prompt": prompt, f"{tag}_out": out, f"{tag}_raw": raw})
            print(f"{tag}: smallest top-2 gap {gap:.2e}")
        else:
            n_bins = io_kw["n_fft"] // 2 + 1
            prompt = torch.rand(clips, prompt_len, n_bins, generator=g)
            out = run_loop(net, (prompt,), n_steps)[0]
            arrays.update({f"{tag}_prompt": prompt, f"{tag}_out": out})
    # what the host mirror must reproduce: the state_dict layout of the default-sized network, the Config defaults
    io = ref.IOSpec.mulaw_io(ref.IOSpec.MuLawIOConfig(input_module_type="embedding"))
    for tag, kw in (("default", {}), ("ln", dict(with_layer_norm=True, num_layers=2))):
        net = tr.SimpleTransformer.from_config(tr.SimpleTransformer.Config(io_spec=io, **kw))
        arrays[f"keys_{tag}"] = json.dumps({k: list(v.shape) for k, v in net.state_dict().items()})
    cfg = tr.SimpleTransformer.Config()
    arrays["config_defaults"] = json.dumps({f: getattr(cfg, f) for f in ("model_dim", "n_heads", "feedforward_dim", "num_layers",
                                                                          "with_layer_norm", "dropout", "input_dropout", "rf")})
    arrays["rf_default"] = np.int64(net.rf)
    arrays["generate_params"] = json.dumps(sorted(net.generate_params))
    arrays["cases"] = json.dumps({tag: [c[0], c[1], c[2], c[3], c[4], c[5]] for tag, c in CASES.items()})
    arrays["gain"] = np.float32(GAIN)
    path = os.path.join(OUT, "transformer.npz")
    # (np.savez, not _compressed: the zip entries then carry no compressor output, and the file is the same bytes on every run)
    np.savez(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()})
    print(f"transformer.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    make()
