"""CPU: the optimizer step's float64 reference (tests/adam_ref.py) against torch, the C ABI of foc_optim_step (struct layout, host-side
refusals), and what focnerf_amd.optim promises without a device: state dicts that go both ways with torch's Adam and GradScaler, the
constructor's refusals, the exports."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adam_ref_is_torch_adam_in_float64(weight_decay):
    rng = np.random.default_rng(0)
    p0 = rng.uniform(-1, 1, 257)
    grads = [rng.standard_normal(257) * 10.0 ** rng.uniform(-6, 2, 257) for _ in range(5)]
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([tp], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=weight_decay)
    p, m, v, step = p0.copy(), np.zeros(257), np.zeros(257), 0.0
    for g in grads:
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        r = adam_ref.adam_step(p, g * 1024.0, m, v, step, scale=1024.0, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=weight_decay)
        assert not r["skipped"]
        p, m, v, step = r["p"], r["m"], r["v"], r["step"]
        st = opt.state[tp]
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        assert float(st["step"]) == step
    assert step == 5.0


def test_adam_ref_skips_on_a_non_finite_grad():
    p, m, v = np.array([0.5, -0.25]), np.array([0.1, 0.2]), np.array([0.3, 0.4])
    for bad in (np.inf, -np.inf, np.nan):
        r = adam_ref.adam_step(p, np.array([1.0, bad]), m, v, 3.0, scale=2.0, lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
        assert r["skipped"] and r["step"] == 3.0
        assert np.array_equal(r["p"], p) and np.array_equal(r["m"], m) and np.array_equal(r["v"], v)
    assert adam_ref.any_nonfinite([np.zeros(3), np.array([np.nan])]) and not adam_ref.any_nonfinite([np.zeros(3)])


def _amp_update_scale(scale, tracker, found_inf, growth_factor, backoff_factor, growth_interval):
    """torch._amp_update_scale_ (ATen/native/cuda/AmpKernels.cu amp_update_scale_cuda_kernel), as coded there, on fp32 scalars."""
    scale = torch.tensor(scale, dtype=torch.float32)
    if found_inf:
        scale = scale * backoff_factor
        tracker = 0
    else:
        successful = tracker + 1
        if successful == growth_interval:
            new_scale = scale * growth_factor
            if torch.isfinite(new_scale):
                scale = new_scale
            tracker = 0
        else:
            tracker = successful
    return float(scale), tracker


def test_scale_rule_is_torchs_amp_update_scale_rule():
    cases = [(65536.0, 0, False, 2.0, 0.5, 2000), (65536.0, 1999, False, 2.0, 0.5, 2000), (65536.0, 1998, False, 2.0, 0.5, 2000),
             (65536.0, 57, True, 2.0, 0.5, 2000), (1024.0, 0, False, 2.0, 0.5, 1), (3.0e38, 0, False, 2.0, 0.5, 1), (3.0, 4, True, 1.7, 0.3, 5),
             (3.0, 4, False, 1.7, 0.3, 5)]
    for c in cases:
        assert adam_ref.scale_rule(*c) == _amp_update_scale(*c), c
    assert adam_ref.scale_rule(3.0e38, 0, False, 2.0, 0.5, 1) == (float(np.float32(3.0e38)), 0)     # a growth to inf is not taken


# ---------------------------------------------------------------- C ABI
def test_optim_structs_match_the_header(tmp_path):
    """The layouts of FocOptimStep / FocOptimTensor against gcc's: tests/test_abi.py test_struct_layout_matches_the_header. Here: the sizes
    the call states about itself and the two limits, as gcc prints them from include/focnerf.h."""
    from focnerf_amd import _lib, optim
    from util import c_header_values
    assert _lib.FocOptimStep._fields_[0][0] == "struct_bytes"
    out = c_header_values(tmp_path, ["sizeof(FocOptimStep)", "sizeof(FocOptimTensor)", "FOC_OPTIM_CHUNK", "FOC_OPTIM_MAX_TENSORS"])
    assert out == [ctypes.sizeof(_lib.FocOptimStep), ctypes.sizeof(_lib.FocOptimTensor), optim.CHUNK, optim.MAX_TENSORS]
    assert out[2:] == [4096, 16]
    assert _lib.lib.foc_abi_version() == 2


def _valid_call(n=2):
    """A call that passes every host check (its pointers are never dereferenced on the device: each test breaks one thing)."""
    from focnerf_amd import _lib
    one = 64                                                        # an aligned non-null address
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


def test_optim_step_refusals_need_no_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib
    step = lib.foc_optim_step

    def refused(call, word):
        rc = step(ctypes.byref(call) if call is not None else None, None)
        msg = lib.foc_last_error()
        assert rc == 1 and word in msg, (rc, msg)

    assert lib.foc_optim_workspace_bytes(0) == 0 and lib.foc_optim_workspace_bytes(17) == 0 and lib.foc_optim_workspace_bytes(-1) == 0
    assert lib.foc_optim_workspace_bytes(1) > 0 and lib.foc_optim_workspace_bytes(16) >= lib.foc_optim_workspace_bytes(1)
    refused(None, b"null step")
    call, arr = _valid_call()
    call.struct_bytes -= 8
    refused(call, b"bytes")
    call, arr = _valid_call()
    call.tensor_bytes += 8
    refused(call, b"bytes")
    for n in (0, 17, -3):
        call, arr = _valid_call()
        call.n_tensors = n
        refused(call, b"n_tensors")
    call, arr = _valid_call()
    call.tensors = None
    refused(call, b"null pointer")
    for field in ("param", "grad", "exp_avg", "exp_avg_sq", "step"):
        call, arr = _valid_call()
        setattr(arr[1], field, None)
        refused(call, b"null pointer")
    for field in ("scale", "growth_tracker", "workspace"):
        call, arr = _valid_call()
        setattr(call, field, None)
        refused(call, b"null pointer")
    call, arr = _valid_call()
    call.scale = call.growth_tracker = None
    call.phase = 1                                                  # the check alone has nothing to write its result for
    refused(call, b"null pointer")
    call, arr = _valid_call()
    arr[0].n = -1
    refused(call, b"negative size")
    for field, value in (("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", 1.5), ("beta2", float("nan"))):
        call, arr = _valid_call()
        setattr(arr[1], field, value)
        refused(call, b"betas")
    for field in ("eps", "lr", "weight_decay"):
        call, arr = _valid_call()
        setattr(arr[0], field, -1e-3)
        refused(call, b"must not be negative")
    call, arr = _valid_call()
    call.workspace_bytes -= 4
    refused(call, b"workspace of")
    call, arr = _valid_call()
    call.grad_scale = 64
    refused(call, b"exclude each other")
    call, arr = _valid_call()
    call.phase = 7
    refused(call, b"phase")


def test_deterministic_mode_refuses_nothing_here(lib_option):
    """FOC_DETERMINISTIC: the same host checks, the same refusals — the kernels have no order-dependent sums to replace."""
    from focnerf_amd import _lib
    lib_option("FOC_DETERMINISTIC", 1)
    call, arr = _valid_call()
    call.workspace_bytes = 0
    assert _lib.lib.foc_optim_step(ctypes.byref(call), None) == 1 and b"workspace of" in _lib.lib.foc_last_error()
    assert b"DETERMINISTIC" not in _lib.lib.foc_last_error()


# ---------------------------------------------------------------- the Python classes, without a device
def _params():
    return [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]


def test_exports():
    import focnerf_amd
    for name in ("optim", "FusedAdam", "LossScaler"):
        assert name in focnerf_amd.__all__ and hasattr(focnerf_amd, name)
    assert focnerf_amd.FusedAdam is focnerf_amd.optim.FusedAdam and focnerf_amd.optim.CHUNK >= 1024
    assert issubclass(focnerf_amd.FusedAdam, torch.optim.Optimizer) and focnerf_amd.FusedAdam._step_supports_amp_scaling is True


def _fill_state(opt):
    """The state a first step creates, on CPU-constructed objects (layout only: key sets and group keys are what is compared)."""
    for group in opt.param_groups:
        for p in group["params"]:
            opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.full_like(p, 0.5), "exp_avg_sq": torch.full_like(p, 0.25)}


def test_state_dicts_go_both_ways_with_torch_adam():
    from focnerf_amd import FusedAdam
    pa, pb = _params(), _params()
    ours = FusedAdam([{"params": pa[:1]}, {"params": pa[1:], "lr": 3e-3, "weight_decay": 0.1}], lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    theirs = torch.optim.Adam([{"params": pb[:1]}, {"params": pb[1:], "lr": 3e-3, "weight_decay": 0.1}], lr=1e-2, betas=(0.9, 0.99), eps=1e-15,
                              fused=True, capturable=True)
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert list(a.keys()) == list(b.keys())
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    _fill_state(ours)
    _fill_state(theirs)
    sa, sb = ours.state_dict(), theirs.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
    assert [g.keys() for g in sa["param_groups"]] == [g.keys() for g in sb["param_groups"]]
    theirs.load_state_dict(sa)
    ours.load_state_dict(sb)
    plain = torch.optim.Adam(_params(), lr=1e-2)                     # the reference trainer's own construction: one group, no flags
    one = FusedAdam(_params(), lr=1e-2)
    _fill_state(one)
    plain.load_state_dict(one.state_dict())
    assert float(plain.state[plain.param_groups[0]["params"][0]]["step"]) == 3.0
    _fill_state(plain)
    one.load_state_dict(plain.state_dict())
    assert torch.equal(one.state[one.param_groups[0]["params"][1]]["exp_avg_sq"], torch.full((2, 3), 0.25))


def test_loss_scaler_speaks_grad_scalers_state_dict():
    from focnerf_amd import LossScaler
    keys = {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    s = LossScaler(init_scale=1024.0, growth_interval=7)
    d = s.state_dict()
    assert set(d) == keys and d["scale"] == 1024.0 and d["growth_interval"] == 7 and d["_growth_tracker"] == 0
    assert s.get_scale() == 1024.0 and not hasattr(s, "update")
    torch_saved = {"scale": 32768.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 321}   # GradScaler.state_dict()
    s.load_state_dict(torch_saved)
    assert s.state_dict() == torch_saved
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = torch.amp.GradScaler("cuda", enabled=True)
    if g.is_enabled():                                              # (on a host without a device torch disables its scaler; its loader then takes nothing)
        g.load_state_dict(s.state_dict())
        assert g.state_dict() == torch_saved
    with pytest.raises(RuntimeError):
        s.load_state_dict({})
    for bad in (dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            LossScaler(**bad)


def test_constructor_refusals_name_the_argument():
    from focnerf_amd import FusedAdam
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(_params(), amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdam(_params(), maximize=True)
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(eps=-1.0), "eps"), (dict(betas=(1.0, 0.9)), "betas"), (dict(betas=(0.9, -0.1)), "betas"),
                     (dict(weight_decay=-0.1), "weight_decay")):
        with pytest.raises(ValueError, match=word):
            FusedAdam(_params(), **kw)
    opt = FusedAdam(_params())
    with pytest.raises(ValueError, match="float32"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))]})
    # grads are looked at when they are there: a step refuses what the kernels do not serve (here, on the host: tensors that are not on a device)
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(RuntimeError, match="sparse grads"):
        opt.step()
    p.grad = torch.zeros(8)[::2]
    with pytest.raises(RuntimeError, match="grads must be float32 and contiguous"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = True
    p.grad = torch.zeros(4)
    with pytest.raises(RuntimeError, match="amsgrad"):
        opt.step()
