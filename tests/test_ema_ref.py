"""CPU: the parameter EMA's rule as tests/ema_ref.py states it (float64 against the fp32 sequence), focnerf_amd.ParameterEMA on CPU tensors
against that statement bit for bit, torch_ema's interface and state dict, the host-side refusals of foc_optim_step_ema and foc_ema_update,
and the `torch_ema` drop-in."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ema_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _params(gen, shapes=((5,), (2, 3), (1,), (4097,))):
    return [torch.nn.Parameter(torch.rand(s, generator=gen) * 2 - 1) for s in shapes]


def _move(params, gen):
    with torch.no_grad():
        for p in params:
            p.add_((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1)


# ---------------------------------------------------------------- the rule
def test_schedule_and_its_crossover():
    """n = 1 -> 2/11; 171/180 meets 0.95 at n = 170: below it the warm-up decides, from it on `decay`."""
    assert ema_ref.decay_at(0.95, 1) == 2 / 11 and ema_ref.decay_at(0.95, None) == 0.95
    assert ema_ref.decay_at(0.95, 169) == 170 / 179 < 0.95
    assert abs(ema_ref.decay_at(0.95, 170) - 0.95) < 1e-15 and ema_ref.decay_at(0.95, 171) == 0.95 == ema_ref.decay_at(0.95, 10 ** 6)
    assert ema_ref.omd_bits(0.95, 1) == int(np.float32(1.0 - 2 / 11).view(np.uint32))


def test_parameter_ema_follows_the_schedule_across_170():
    """num_updates = 168 through load_state_dict, four updates (n = 169 .. 172). With s = 0 and p = -1 the rule leaves s = -omd exactly:
    the fp32 bits of the omd the class used, against Python's own double arithmetic."""
    from focnerf_amd import ParameterEMA
    p = torch.nn.Parameter(torch.tensor([-1.0]))
    ema = ParameterEMA([p], 0.95)
    ema.load_state_dict({"decay": 0.95, "num_updates": 168, "shadow_params": [torch.zeros(1)], "collected_params": None})
    for n in (169, 170, 171, 172):
        ema.shadow_params[0].zero_()
        ema.update()
        want = np.float32(1.0 - min(0.95, (1 + n) / (10 + n)))
        got = (-ema.shadow_params[0]).numpy()
        assert got.view(np.uint32)[0] == want.view(np.uint32), (n, float(got[0]), float(want))
        assert ema.num_updates == n
    assert ema_ref.omd_bits(0.95, 172) == ema_ref.omd_bits(0.95, None) != ema_ref.omd_bits(0.95, 169)


def test_fp32_sequence_within_three_roundings_of_float64():
    rng = np.random.default_rng(0)
    for n in (1, 2, 50, 169, 170, 171, None):
        s = rng.uniform(-1, 1, 10000).astype(np.float32)
        p = (s + rng.standard_normal(10000) * 10.0 ** rng.uniform(-6, 0, 10000)).astype(np.float32)
        o = ema_ref.omd(0.95, n)
        err = np.abs(ema_ref.update_f32(s, p, o).astype(np.float64) - ema_ref.update_f64(s, p, o))
        b = ema_ref.bound(s, p, o)
        assert (err <= b).all(), (n, float((err / np.maximum(b, 1e-300)).max()))
    assert np.array_equal(ema_ref.update_f32(s, s, o), s), "a shadow equal to its parameter stays"


def test_parameter_ema_on_cpu_is_the_fp32_statement():
    from focnerf_amd import ParameterEMA
    gen = torch.Generator().manual_seed(1)
    params = _params(gen)
    ema = ParameterEMA(params, 0.95)
    assert ema.num_updates == 0 and all(torch.equal(s, p) and s is not p and not s.requires_grad for s, p in zip(ema.shadow_params, params))
    shadows = [s.numpy().copy() for s in ema.shadow_params]
    for it in range(5):
        _move(params, gen)
        ema.update()
        shadows, n = ema_ref.run(shadows, [[p.detach().numpy() for p in params]], 0.95, n0=it)
        assert ema.num_updates == n == it + 1
        for s, r in zip(ema.shadow_params, shadows):
            assert np.array_equal(s.numpy().view(np.uint32), r.view(np.uint32)), it
    ema.update(params)                                               # explicit parameters, as torch_ema allows
    assert ema.num_updates == 6
    with pytest.raises(ValueError, match="Number of parameters"):
        ema.update(params[:2])
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="Decay must be between 0 and 1"):
            ParameterEMA(params, bad)


def test_constant_decay_without_num_updates():
    from focnerf_amd import ParameterEMA
    gen = torch.Generator().manual_seed(2)
    params = _params(gen)
    ema = ParameterEMA(params, 0.9, use_num_updates=False)
    shadows = [s.numpy().copy() for s in ema.shadow_params]
    for it in range(3):
        _move(params, gen)
        ema.update()
        shadows, n = ema_ref.run(shadows, [[p.detach().numpy() for p in params]], 0.9, use_num_updates=False)
        assert n is None and ema.num_updates is None
        for s, r in zip(ema.shadow_params, shadows):
            assert np.array_equal(s.numpy().view(np.uint32), r.view(np.uint32))
    assert ema.state_dict()["num_updates"] is None


def test_store_copy_to_restore_keep_the_exact_bits():
    from focnerf_amd import ParameterEMA
    gen = torch.Generator().manual_seed(3)
    params = _params(gen)
    ema = ParameterEMA(params, 0.95)
    _move(params, gen)
    ema.update()
    raw = [p.detach().clone() for p in params]
    avg = [s.clone() for s in ema.shadow_params]
    assert not any(torch.equal(r, a) for r, a in zip(raw, avg))
    with pytest.raises(RuntimeError, match="store"):
        ema.restore()
    ema.store()
    ema.copy_to()
    assert all(torch.equal(_bits(p), _bits(a)) for p, a in zip(params, avg)) and all(p.requires_grad for p in params)
    ema.restore()
    assert all(torch.equal(_bits(p), _bits(r)) for p, r in zip(params, raw))
    with ema.average_parameters():
        assert all(torch.equal(_bits(p), _bits(a)) for p, a in zip(params, avg))
    assert all(torch.equal(_bits(p), _bits(r)) for p, r in zip(params, raw))
    with pytest.raises(KeyError):                                    # an exception inside the block still restores
        with ema.average_parameters():
            raise KeyError("x")
    assert all(torch.equal(_bits(p), _bits(r)) for p, r in zip(params, raw))
    assert all(torch.equal(_bits(s), _bits(a)) for s, a in zip(ema.shadow_params, avg)), "evaluation leaves the averages alone"


def test_state_dict_is_torch_emas():
    from focnerf_amd import ParameterEMA
    gen = torch.Generator().manual_seed(4)
    params = _params(gen)
    ema = ParameterEMA(params, 0.95)
    for _ in range(3):
        _move(params, gen)
        ema.update()
    ema.store()
    d = ema.state_dict()
    assert list(d) == ["decay", "num_updates", "shadow_params", "collected_params"]
    assert d["decay"] == 0.95 and d["num_updates"] == 3 and type(d["num_updates"]) is int
    assert isinstance(d["shadow_params"], list) and isinstance(d["collected_params"], list) and len(d["shadow_params"]) == len(params)
    assert all(isinstance(t, torch.Tensor) for t in d["shadow_params"] + d["collected_params"])
    other_params = _params(gen)                                      # (kept alive: the class holds weak references, as torch_ema does)
    other = ParameterEMA(other_params, 0.5)
    other.load_state_dict(d)
    assert other.decay == 0.95 and other.num_updates == 3
    assert all(torch.equal(_bits(a), _bits(b)) and a is not b for a, b in zip(other.shadow_params, ema.shadow_params))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other.collected_params, ema.collected_params))
    _move(params, gen)                                               # both continue alike from the loaded state
    ema.update()
    other.update(params)
    assert other.num_updates == 4 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other.shadow_params, ema.shadow_params))
    # a dict written by hand in torch_ema's layout (float64 tensors: the loader casts to the parameters' dtype, as torch_ema does)
    hand = {"decay": 0.9, "num_updates": 7, "shadow_params": [torch.full(p.shape, 0.25, dtype=torch.float64) for p in params], "collected_params": None}
    other.load_state_dict(hand)
    assert other.decay == 0.9 and other.num_updates == 7 and other.collected_params is None
    assert all(s.dtype == torch.float32 and bool((s == 0.25).all()) for s in other.shadow_params)
    hand["num_updates"] = None
    other.load_state_dict(hand)
    assert other.num_updates is None
    with pytest.raises(ValueError, match="wrong number of parameters"):
        other.load_state_dict(dict(hand, shadow_params=hand["shadow_params"][:1]))
    with pytest.raises(ValueError, match="Decay"):
        other.load_state_dict(dict(hand, decay=2.0))
    ema.to(dtype=torch.float64)
    assert all(s.dtype == torch.float64 for s in ema.shadow_params + ema.collected_params) and ema.num_updates == 4


def test_exports_and_dropin():
    import focnerf_amd
    assert "ParameterEMA" in focnerf_amd.__all__ and "ema" in focnerf_amd.__all__ and focnerf_amd.ParameterEMA is focnerf_amd.ema.ParameterEMA
    dropin = os.path.join(REPO, "focnerf_amd", "dropin")
    saved = sys.modules.pop("torch_ema", None)
    sys.path.insert(0, dropin)
    try:
        from torch_ema import ExponentialMovingAverage
        assert ExponentialMovingAverage is focnerf_amd.ParameterEMA
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("torch_ema", None)
        if saved is not None:
            sys.modules["torch_ema"] = saved


# ---------------------------------------------------------------- C ABI: refusals come from the host, before any launch
def _valid_step(n=2):
    """A foc_optim_step call that passes every host check (its pointers are never dereferenced: each test breaks one thing)."""
    from focnerf_amd import _lib
    one = 64
    arr = (_lib.FocOptimTensor * n)()
    for d in arr:
        d.param = d.grad = d.exp_avg = d.exp_avg_sq = d.step = one
        d.n, d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = 8, 1e-2, 0.9, 0.99, 1e-15, 0.0
    call = _lib.FocOptimStep()
    call.struct_bytes, call.tensor_bytes = ctypes.sizeof(_lib.FocOptimStep), ctypes.sizeof(_lib.FocOptimTensor)
    call.n_tensors, call.tensors = n, arr
    call.scale = call.growth_tracker = one
    call.growth_factor, call.backoff_factor, call.growth_interval = 2.0, 0.5, 2000
    call.workspace, call.workspace_bytes = one, _lib.lib.foc_optim_workspace_bytes(n)
    return call, arr


def test_optim_step_ema_refusals_need_no_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib
    assert lib.foc_abi_version() == 2 and lib.foc_optim_workspace_bytes(16) == 4 * (64 + 8 * 32), "the workspace has not grown"

    def refused(word, call, shadow, decay=0.95, counter=64, advance=1):
        rc = lib.foc_optim_step_ema(ctypes.byref(call) if call is not None else None, shadow, decay, counter, advance, None)
        msg = lib.foc_last_error()
        assert rc == 1 and word in msg, (rc, msg, word)

    shadow = (ctypes.c_uint64 * 2)(64, 0)
    refused(b"null step", None, shadow)
    call, arr = _valid_step()
    refused(b"null pointer (shadow)", call, None)
    for decay in (-0.01, 1.01, float("nan"), float("inf")):
        refused(b"decay must lie in [0, 1]", call, shadow, decay=decay)
    refused(b"num_updates must be 8-byte aligned", call, shadow, counter=68)
    refused(b"shadow must be 4-byte aligned", call, (ctypes.c_uint64 * 2)(0, 66))
    call.phase = 1
    refused(b"advance belongs to the decide or step phase", call, shadow)
    # everything foc_optim_step refuses, with its message
    call, arr = _valid_step()
    call.struct_bytes -= 8
    refused(b"bytes", call, shadow)
    for n in (0, 17, -3):
        call, arr = _valid_step()
        call.n_tensors = n
        refused(b"n_tensors", call, shadow)
    call, arr = _valid_step()
    arr[1].exp_avg = None
    refused(b"null pointer", call, shadow)
    call, arr = _valid_step()
    arr[0].n = -1
    refused(b"negative size", call, shadow)
    call, arr = _valid_step()
    call.workspace_bytes -= 4
    refused(b"workspace of", call, shadow)
    call, arr = _valid_step()
    arr[1].grad = 66
    refused(b"4-byte aligned", call, shadow)
    call, arr = _valid_step()
    call.scale = call.growth_tracker = None
    call.phase = 2                                                   # a decision without a scaler, with or without shadows
    refused(b"null pointer", call, None)


def test_ema_update_refusals_need_no_gpu(lib_option):
    from focnerf_amd import _lib
    lib = _lib.lib
    ws_bytes = lib.foc_optim_workspace_bytes(16)

    def refused(word, param=(64, 128), shadow=(256, 512), n=(8, 0), n_tensors=2, decay=0.95, counter=64, workspace=1024, nbytes=ws_bytes):
        arrays = [None if a is None else (t * len(a))(*a) for a, t in ((param, ctypes.c_uint64), (shadow, ctypes.c_uint64), (n, ctypes.c_int64))]
        rc = lib.foc_ema_update(*arrays, n_tensors, decay, counter, 1, workspace, nbytes, None)
        msg = lib.foc_last_error()
        assert rc == 1 and word in msg, (rc, msg, word)

    for which in ("param", "shadow", "n"):
        refused(b"null pointer (param, shadow and n", **{which: None})
    many = tuple(64 * (k + 1) for k in range(17))
    for k in (0, 17, -1):
        refused(b"n_tensors must be 1 .. 16", param=many, shadow=many, n=(1,) * 17, n_tensors=k)
    for decay in (-1e-9, 1.5, float("nan"), float("-inf")):
        refused(b"decay must lie in [0, 1]", decay=decay)
    refused(b"null pointer (tensor 1)", param=(64, 0))
    refused(b"null pointer (tensor 0)", shadow=(0, 512))
    refused(b"negative size (tensor 1: -5)", n=(8, -5))
    refused(b"tensor 1: pointers must be 4-byte aligned", param=(64, 130))
    refused(b"tensor 0: pointers must be 4-byte aligned", shadow=(257, 512))
    refused(b"num_updates must be 8-byte aligned", counter=68)
    refused(b"null pointer (workspace)", workspace=None)
    refused(b"workspace must be 4-byte aligned", workspace=1026)
    refused(b"workspace of", nbytes=ws_bytes - 4)
    lib_option("FOC_DETERMINISTIC", 1)                               # the same refusals: there is no order-dependent sum to replace
    refused(b"workspace of", nbytes=0)
    assert b"DETERMINISTIC" not in lib.foc_last_error()
