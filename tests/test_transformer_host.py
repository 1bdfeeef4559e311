"""SimpleTransformer host mirror and C ABI checks that need no GPU (tests/golden/transformer.npz comes from the reference)."""
import ctypes as C
import json

import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests.helpers import golden

G = golden("transformer.npz")


def mulaw(**kw):
    return mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig(input_module_type="embedding", **kw))


def tiny(io=None, **kw):
    kw = {**dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=16), **kw}
    return mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=io or mulaw(mlp_dim=32), **kw))


def test_config_defaults_rf_and_generate_params_match_the_reference():
    cfg = mmk.SimpleTransformer.Config()
    want = json.loads(str(G["config_defaults"]))
    assert {k: getattr(cfg, k) for k in want} == want
    for k in ("model_dim", "n_heads", "feedforward_dim", "num_layers", "rf"):
        assert type(getattr(cfg, k)) is int
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=mulaw()))
    assert net.rf == int(G["rf_default"]) == 64
    assert sorted(net.generate_params) == json.loads(str(G["generate_params"]))
    assert mmk.networks.SimpleTransformer is mmk.SimpleTransformer and mmk.PositionalEncoding is not None


@pytest.mark.parametrize("tag,kw", [("default", {}), ("ln", dict(with_layer_norm=True, num_layers=2))])
def test_state_dict_keys_and_shapes_equal_the_reference(tag, kw):
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=mulaw(), **kw))
    mine = {k: list(v.shape) for k, v in net.state_dict().items()}
    want = json.loads(str(G[f"keys_{tag}"]))
    assert list(mine) == list(want)
    assert mine == want
    assert want["pe.pe"] == [2048, 1, net.config.model_dim]


def test_checkpoint_round_trip(tmp_path):
    net = tiny(with_layer_norm=True)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.rand_like(p))
    path = mmk.save_network(str(tmp_path / "tr.ckpt"), net)
    back = mmk.load_network(path)
    assert type(back) is mmk.SimpleTransformer and back.config.serialize() == net.config.serialize()
    for (k, a), (k2, b) in zip(net.state_dict().items(), back.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    assert "SimpleTransformer.Config" in net.config.serialize()


def test_training_forward_is_the_torch_graph():
    net = tiny().train()
    x = torch.randint(0, 256, (2, 16))
    with torch.enable_grad():
        out = net((x,))[0]
    assert out.shape == (2, 16, 256) and out.requires_grad      # (the MLP divides by its learned temperature in training mode too)


def test_refusals_name_the_option():
    # the default mulaw_io (framed_linear) fails in from_config, as in the reference
    with pytest.raises(ValueError, match="frame_size"):
        tiny(io=mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig()))
    # a temperature with a continuous head: the reference's Sequential takes no keyword
    mag = tiny(io=mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=64, hop_length=16)), rf=8).eval()
    with pytest.raises(TypeError, match="temperature"):
        mag((torch.rand(2, 8, 33),), temperature=1.0)
    with pytest.raises(TypeError, match="temperature"):
        mag.generate_block((torch.rand(2, 12, 33),), 8, 4, temperature=1.0)
    # a prompt shorter than rf: the reference's window slice is empty
    net = tiny().eval()
    with pytest.raises(ValueError, match="rf=16"):
        net.generate_block((torch.zeros(2, 20, dtype=torch.long),), 10, 10)
    with pytest.raises(ValueError, match="rf=16"):
        net.generate_step((torch.zeros(2, 10, dtype=torch.long),), t=10)
    # IO outside the covered pair
    with pytest.raises(NotImplementedError, match="does not cover: MLP head with more than 4 hidden layers"):
        tiny(io=mulaw(n_mlp_layers=5))._describe(1)
    io = mulaw()
    two = mmk.IOSpec(inputs=io.inputs, targets=io.targets + io.targets)
    with pytest.raises(NotImplementedError, match="does not cover: 1 inputs and 2 targets"):
        tiny(io=two)._describe(1)
    mixed = mmk.IOSpec(inputs=mulaw().inputs, targets=mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=64, hop_length=16)).targets)
    with pytest.raises(NotImplementedError, match="class indices in with frames out"):
        tiny(io=mixed)._describe(1)
    # ... and what is covered describes itself
    c = tiny(io=mulaw(n_mlp_layers=2), with_layer_norm=True)._describe(7)
    assert (c.in_kind, c.in_classes, c.head_kind, c.out_dim, c.mlp_n_hidden, c.learn_temp, c.final_norm, c.max_batch) == (0, 256, 0, 256, 2, 1, 1, 7)
    c = mag._describe(3)
    assert (c.in_kind, c.in_dim, c.head_kind, c.out_dim, c.out_abs, c.final_norm) == (1, 33, 1, 33, 1, 0)


def test_eval_generation_off_the_device_raises():
    net = tiny().eval()
    x = torch.randint(0, 256, (2, 16))
    with pytest.raises(RuntimeError, match="MI355X"):
        net((x,))
    with pytest.raises(RuntimeError, match="MI355X"):
        net.generate_step((x,), t=16)
    with pytest.raises(RuntimeError, match="MI355X"):
        net.before_generate((x,), None)
    with pytest.raises(RuntimeError, match="MI355X"):
        net.generate_block((torch.zeros(2, 20, dtype=torch.long),), 16, 4)


def _cfg(**kw):
    c = native.TransformerConfig()
    c.model_dim, c.n_heads, c.feedforward_dim, c.num_layers, c.rf, c.max_batch = 64, 4, 128, 2, 16, 4
    c.in_kind, c.in_classes, c.head_kind, c.out_dim = 0, 256, 0, 256
    c.mlp_hidden, c.mlp_n_hidden, c.mlp_act, c.learn_temp, c.min_temp = 32, 1, native.ACT["Mish"], 1, 1e-4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_abi_argument_validation_needs_no_gpu():
    lib = native.load_library()
    assert lib.mmk_config_bytes(3) == C.sizeof(native.TransformerConfig)
    handle = native.vp()
    for kw, field in ((dict(n_heads=3), b"n_heads"), (dict(n_heads=32), b"head_dim"), (dict(model_dim=512, n_heads=2), b"head_dim"),
                      (dict(model_dim=56), b"model_dim"), (dict(model_dim=2048, n_heads=16), b"model_dim"), (dict(rf=2049), b"rf"),
                      (dict(rf=0), b"rf"), (dict(num_layers=17), b"num_layers"), (dict(feedforward_dim=4097), b"feedforward_dim"),
                      (dict(max_batch=513), b"max_batch")):
        assert lib.mmk_tr_plan_create(C.byref(_cfg(**kw)), C.byref(handle)) == -1, kw
        assert field in lib.mmk_last_error(), (kw, lib.mmk_last_error())
    assert lib.mmk_tr_plan_create(C.byref(_cfg(head_kind=1)), C.byref(handle)) == -3
    assert lib.mmk_tr_plan_create(C.byref(_cfg(model_dim=1024, n_heads=8, rf=2048)), C.byref(handle)) == 0
    lib.mmk_tr_plan_destroy(handle)
    assert lib.mmk_tr_plan_create(C.byref(_cfg()), C.byref(handle)) == 0
    assert lib.mmk_tr_workspace_bytes(handle) > 0
    buf = (C.c_int64 * 64)()
    assert lib.mmk_tr_generate(handle, 2, buf, 32, 1, 16, 4, None, None, None) == -5
    assert b"not committed" in lib.mmk_last_error()
    assert lib.mmk_tr_step(handle, 2, buf, 16, 1, buf, 1, None, None, None) == -5
    lib.mmk_tr_plan_destroy(handle)
