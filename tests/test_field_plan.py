"""Which fused kernels serve a network: `field.field_plan`'s verdicts across network shapes, attribute changes and switches, on the CPU.

Each row builds one network (`network.NeRFNetwork` = "ff", `network_foc.NeRFNetwork` = "foc") on the meta device, changes at most one
attribute or turns at most one switch off, and compares the plan's seven verdicts with EXPECTED. The table was generated at the commit
before `field_plan` existed, from the nine per-path predicates it replaced (the fused training forward's taken behind the field node's
and the tail's, as its caller took it), with their per-call conditions (GPU tensor, flat input, autocast, no autograd) taken as met; the
row of that commit's Python-side switch for the fused training forward is the FOC_FIELD_FWD_FUSED=0 row here. PLAN_DIFFERS lists the rows
where a rule the old predicates stated differently is now stated once; no constructor builds any of them.
"""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _have_lib():
    return os.path.exists(os.path.join(os.path.dirname(HERE), "focnerf_amd", "libfocnerf_hip.so"))


pytestmark = pytest.mark.skipif(not _have_lib(), reason="libfocnerf_hip.so not built")

VERDICTS = ("field", "train_forward", "tail", "infer", "occ", "native_loop", "head")


def _network(kind, sigma_layers=2, sigma_hidden=64, colour_layers=None, colour_hidden=64):
    """colour_layers: layers of the colour FFMLP itself (network_foc's constructor takes one more)."""
    from focnerf_amd.network import NeRFNetwork
    from focnerf_amd.network_foc import NeRFNetwork as FocNetwork
    with torch.device("meta"):
        if kind == "ff":
            return NeRFNetwork(num_layers=sigma_layers, hidden_dim=sigma_hidden, num_layers_color=colour_layers or 3, hidden_dim_color=colour_hidden)
        return FocNetwork(num_layers=sigma_layers, hidden_dim=sigma_hidden, num_layers_color=(colour_layers or 2) + 1, hidden_dim_color=colour_hidden)


def _set(**attrs):
    """A row's attribute change: {"sub.attr": value} on the network (a module value replaces the sub-module)."""
    def apply(m):
        for path, value in attrs.items():
            owner, _, name = path.rpartition(".")
            setattr(m.get_submodule(owner) if owner else m, name, value)
    return apply


ATTRIBUTES = {
    "encoder not a hash grid": _set(encoder=torch.nn.Identity()),
    "encoder input_dim 2": _set(**{"encoder.input_dim": 2}),
    "encoder level_dim 4": _set(**{"encoder.level_dim": 4}),
    "encoder output 48 wide": _set(**{"encoder.output_dim": 48}),
    "gridtype tiled": _set(**{"encoder.gridtype": "tiled", "encoder.gridtype_id": 1}),
    "align_corners": _set(**{"encoder.align_corners": True}),
    "interpolation smoothstep": _set(**{"encoder.interpolation": "smoothstep", "encoder.interp_id": 1}),
    "sigma_net not an FFMLP": _set(sigma_net=torch.nn.Identity()),
    "sigma input 48": _set(**{"encoder.output_dim": 48, "sigma_net.input_dim": 48}),
    "sigma input 80": _set(**{"encoder.output_dim": 80, "sigma_net.input_dim": 80}),
    "sigma layers 5": _set(**{"sigma_net.num_layers": 5}),
    "sigma output 32 wide": _set(**{"sigma_net.padded_output_dim": 32}),
    "sigma output activation relu": _set(**{"sigma_net.output_activation": 0}),
    "sigma activation sigmoid": _set(**{"sigma_net.activation": 3}),
    "sigma activation none": _set(**{"sigma_net.activation": 6}),
    "color_net not an FFMLP": _set(color_net=torch.nn.Identity()),
    "colour input 64": _set(**{"color_net.input_dim": 64, "in_dim_color": 64}),
    "colour output 32 wide": _set(**{"color_net.padded_output_dim": 32}),
    "colour activation sigmoid": _set(**{"color_net.activation": 3}),
    "colour activation none": _set(**{"color_net.activation": 6}),
    "both activations none": _set(**{"sigma_net.activation": 6, "color_net.activation": 6}),
    "encoder_dir not SH": _set(encoder_dir=torch.nn.Identity()),
    "SH degree 3": _set(**{"encoder_dir.degree": 3}),
    "geo_feat_dim 14": _set(geo_feat_dim=14),
    "yolo_encoding_dim 8": _set(yolo_encoding_dim=8),
    "bg_radius 1": _set(bg_radius=1),
    "density_scale 2": _set(density_scale=2),
}

# (name, kind): environment variables are read per call, library options through the `lib_option` fixture
SWITCHES = (("FOC_FUSED_FIELD", "env"), ("FOC_FUSED_HEAD", "env"), ("FOC_FUSED_TAIL", "env"), ("FOC_FUSED_INFER", "env"),
            ("FOC_FUSED_OCC", "env"), ("FOC_RENDER_NATIVE", "env"), ("FOC_MLP_BWD_FUSED", "lib"), ("FOC_FIELD_FWD_FUSED", "lib"))


def rows(kind, group):
    """(row id, network factory, attribute change or None, switch or None) of one group of the table."""
    if group == "shapes":
        for sl in (2, 3, 4):
            for sh in (32, 64, 128):
                for cl in (2, 3, 4):
                    for ch in (64, 128):
                        yield (f"{kind} sigma {sl}x{sh} colour {cl}x{ch}",
                               lambda sl=sl, sh=sh, cl=cl, ch=ch: _network(kind, sl, sh, cl, ch), None, None)
    elif group == "attributes":
        for name, change in ATTRIBUTES.items():
            yield f"{kind} {name}", lambda: _network(kind), change, None
    else:
        for switch in SWITCHES:
            yield f"{kind} {switch[0]}=0", lambda: _network(kind), None, switch


def _verdicts(plan):
    return "".join("1" if getattr(plan, v) else "0" for v in VERDICTS)


@pytest.mark.parametrize("group", ["shapes", "attributes", "switches"])
@pytest.mark.parametrize("kind", ["ff", "foc"])
def test_decision_table(kind, group, monkeypatch, lib_option):
    from focnerf_amd.field import field_plan
    wrong = []
    for row, make, change, switch in rows(kind, group):
        m = make()
        if change is not None:
            change(m)
        if switch is not None:
            if switch[1] == "env":
                monkeypatch.setenv(switch[0], "0")
            else:
                lib_option(switch[0], 0)
        got = _verdicts(field_plan(m))
        want = PLAN_DIFFERS.get(row, (EXPECTED[row], None))[0]
        if got != want:
            wrong.append(f"{row}: {dict(zip(VERDICTS, got))} != {dict(zip(VERDICTS, want))}")
        if switch is not None:
            if switch[1] == "env":
                monkeypatch.delenv(switch[0])
            else:
                lib_option(switch[0], 1)
    assert not wrong, "\n".join(wrong)


def test_plan_differs_only_where_stated():
    """Every PLAN_DIFFERS row exists in EXPECTED and really differs from it."""
    for row, (verdicts, why) in PLAN_DIFFERS.items():
        assert row in EXPECTED and EXPECTED[row] != verdicts and why, row


def test_switches_take_effect_at_the_next_plan(monkeypatch, lib_option):
    """The plan is built per call, not kept: a switch flipped between two calls reaches the second one."""
    from focnerf_amd.field import field_plan
    m = _network("ff")
    assert field_plan(m).infer and field_plan(m).train_forward
    monkeypatch.setenv("FOC_FUSED_INFER", "0")
    assert not field_plan(m).infer
    monkeypatch.delenv("FOC_FUSED_INFER")
    lib_option("FOC_FIELD_FWD_FUSED", 0)
    plan = field_plan(m)
    assert plan.infer and not plan.train_forward


def test_plan_carries_the_kernel_arguments():
    import numpy as np
    from focnerf_amd.field import field_plan
    from focnerf_amd.gridencoder import GridSpec
    m = _network("foc", colour_layers=3)
    plan = field_plan(m)
    assert plan.grid == GridSpec(float(np.log2(m.encoder.per_level_scale)), 16, 0, False, 0) and plan.levels == 16
    assert (plan.sigma.input_dim, plan.sigma.hidden_dim, plan.sigma.num_layers) == (32, 64, 2)
    assert (plan.colour.input_dim, plan.colour.hidden_dim, plan.colour.num_layers) == (48, 64, 3) and plan.uses_object_feature
    assert plan.colour.blob_numel() == m.color_net.weights.numel()


def _colour_branch_case(case):
    """A CPU network, its points and a colour branch with one thing wrong (`case`)."""
    from focnerf_amd.field import field_plan, _half_of
    from focnerf_amd.network_foc import NeRFNetwork as FocNetwork
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    m = (FocNetwork if case.startswith("foc") else NeRFNetwork)()
    plan = field_plan(m)
    N, T = 4, 8
    x = torch.rand(N * T, 3)
    ray_sh = torch.zeros(N, 16, dtype=torch.half)
    obj = torch.zeros(16) if plan.uses_object_feature else None
    wc, c_width = _half_of(m.color_net.weights), 4
    if case == "ray_sh rows":
        ray_sh = torch.zeros(N + 1, 16, dtype=torch.half)
    elif case == "ray_sh dtype":
        ray_sh = ray_sh.float()
    elif case == "ray_sh strided":
        ray_sh = torch.zeros(16, N, dtype=torch.half).t()
    elif case == "c_width":
        c_width = 8
    elif case == "foc without object feature":
        obj = None
    elif case == "object feature on a 32-wide net":
        obj = torch.zeros(16)
    elif case == "foc object feature size":
        obj = torch.zeros(15)
    elif case == "colour blob size":
        wc = wc[:-1]
    else:
        assert case.endswith("as it should be")
    return m, plan, x, (wc, plan.colour, ray_sh, T, c_width, obj)


@pytest.mark.parametrize("case", ["ray_sh rows", "ray_sh dtype", "ray_sh strided", "c_width", "foc without object feature",
                                  "object feature on a 32-wide net", "foc object feature size", "colour blob size"])
def test_fused_training_forward_checks_its_colour_branch_before_any_launch(case):
    """CPU tensors: a launch would fail in the library's argument checks ("expected a CUDA(HIP) tensor"). The colour branch's own checks
    come first, so the error names what is wrong with it."""
    from focnerf_amd.field import hashgrid_mlp
    m, plan, x, colour = _colour_branch_case(case)
    with pytest.raises(RuntimeError, match="colour branch"):
        hashgrid_mlp(m.encoder, m.sigma_net, x, None, colour=colour)


@pytest.mark.parametrize("case", ["ff branch as it should be", "foc branch as it should be"])
def test_a_sound_colour_branch_passes_the_checks(case):
    """The same call with nothing wrong gets past the colour branch's checks, to the first launch (which refuses CPU tensors)."""
    from focnerf_amd.field import hashgrid_mlp
    m, plan, x, colour = _colour_branch_case(case)
    with pytest.raises(RuntimeError, match="CUDA"):
        hashgrid_mlp(m.encoder, m.sigma_net, x, None, colour=colour)


# generated at the parent commit from the old predicates (see the module docstring); verdict order: VERDICTS
EXPECTED = {
    'ff sigma 2x32 colour 2x64': '1010101',
    'ff sigma 2x32 colour 2x128': '1000001',
    'ff sigma 2x32 colour 3x64': '1010101',
    'ff sigma 2x32 colour 3x128': '1000001',
    'ff sigma 2x32 colour 4x64': '1000001',
    'ff sigma 2x32 colour 4x128': '1000001',
    'ff sigma 2x64 colour 2x64': '1111111',
    'ff sigma 2x64 colour 2x128': '1000001',
    'ff sigma 2x64 colour 3x64': '1111111',
    'ff sigma 2x64 colour 3x128': '1000001',
    'ff sigma 2x64 colour 4x64': '1000001',
    'ff sigma 2x64 colour 4x128': '1000001',
    'ff sigma 2x128 colour 2x64': '0010001',
    'ff sigma 2x128 colour 2x128': '0000001',
    'ff sigma 2x128 colour 3x64': '0010001',
    'ff sigma 2x128 colour 3x128': '0000001',
    'ff sigma 2x128 colour 4x64': '0000001',
    'ff sigma 2x128 colour 4x128': '0000001',
    'ff sigma 3x32 colour 2x64': '1010101',
    'ff sigma 3x32 colour 2x128': '1000001',
    'ff sigma 3x32 colour 3x64': '1010101',
    'ff sigma 3x32 colour 3x128': '1000001',
    'ff sigma 3x32 colour 4x64': '1000001',
    'ff sigma 3x32 colour 4x128': '1000001',
    'ff sigma 3x64 colour 2x64': '1010101',
    'ff sigma 3x64 colour 2x128': '1000001',
    'ff sigma 3x64 colour 3x64': '1111111',
    'ff sigma 3x64 colour 3x128': '1000001',
    'ff sigma 3x64 colour 4x64': '1000001',
    'ff sigma 3x64 colour 4x128': '1000001',
    'ff sigma 3x128 colour 2x64': '0010001',
    'ff sigma 3x128 colour 2x128': '0000001',
    'ff sigma 3x128 colour 3x64': '0010001',
    'ff sigma 3x128 colour 3x128': '0000001',
    'ff sigma 3x128 colour 4x64': '0000001',
    'ff sigma 3x128 colour 4x128': '0000001',
    'ff sigma 4x32 colour 2x64': '1010101',
    'ff sigma 4x32 colour 2x128': '1000001',
    'ff sigma 4x32 colour 3x64': '1010101',
    'ff sigma 4x32 colour 3x128': '1000001',
    'ff sigma 4x32 colour 4x64': '1000001',
    'ff sigma 4x32 colour 4x128': '1000001',
    'ff sigma 4x64 colour 2x64': '1010101',
    'ff sigma 4x64 colour 2x128': '1000001',
    'ff sigma 4x64 colour 3x64': '1010101',
    'ff sigma 4x64 colour 3x128': '1000001',
    'ff sigma 4x64 colour 4x64': '1000001',
    'ff sigma 4x64 colour 4x128': '1000001',
    'ff sigma 4x128 colour 2x64': '0010001',
    'ff sigma 4x128 colour 2x128': '0000001',
    'ff sigma 4x128 colour 3x64': '0010001',
    'ff sigma 4x128 colour 3x128': '0000001',
    'ff sigma 4x128 colour 4x64': '0000001',
    'ff sigma 4x128 colour 4x128': '0000001',
    'ff encoder not a hash grid': '0010001',
    'ff encoder input_dim 2': '0010001',
    'ff encoder level_dim 4': '0010001',
    'ff encoder output 48 wide': '0010001',
    'ff gridtype tiled': '1111101',
    'ff align_corners': '1111101',
    'ff interpolation smoothstep': '1111101',
    'ff sigma_net not an FFMLP': '0010000',
    'ff sigma input 48': '1010101',
    'ff sigma input 80': '0010001',
    'ff sigma layers 5': '0010001',
    'ff sigma output 32 wide': '0010001',
    'ff sigma output activation relu': '1011111',
    'ff sigma activation sigmoid': '0010001',
    'ff sigma activation none': '1010001',
    'ff color_net not an FFMLP': '1000000',
    'ff colour input 64': '1000000',
    'ff colour output 32 wide': '1000001',
    'ff colour activation sigmoid': '1000001',
    'ff colour activation none': '1010001',
    'ff both activations none': '1111111',
    'ff encoder_dir not SH': '1000000',
    'ff SH degree 3': '1111110',
    'ff geo_feat_dim 14': '1000000',
    'ff yolo_encoding_dim 8': '1111111',
    'ff bg_radius 1': '1111011',
    'ff density_scale 2': '1111101',
    'ff FOC_FUSED_FIELD=0': '0010001',
    'ff FOC_FUSED_HEAD=0': '1111110',
    'ff FOC_FUSED_TAIL=0': '1001011',
    'ff FOC_FUSED_INFER=0': '1110101',
    'ff FOC_FUSED_OCC=0': '1111011',
    'ff FOC_RENDER_NATIVE=0': '1111101',
    'ff FOC_MLP_BWD_FUSED=0': '0010001',
    'ff FOC_FIELD_FWD_FUSED=0': '1011111',
    'foc sigma 2x32 colour 2x64': '1010001',
    'foc sigma 2x32 colour 2x128': '1000001',
    'foc sigma 2x32 colour 3x64': '1010001',
    'foc sigma 2x32 colour 3x128': '1000001',
    'foc sigma 2x32 colour 4x64': '1000001',
    'foc sigma 2x32 colour 4x128': '1000001',
    'foc sigma 2x64 colour 2x64': '1111001',
    'foc sigma 2x64 colour 2x128': '1000001',
    'foc sigma 2x64 colour 3x64': '1111001',
    'foc sigma 2x64 colour 3x128': '1000001',
    'foc sigma 2x64 colour 4x64': '1000001',
    'foc sigma 2x64 colour 4x128': '1000001',
    'foc sigma 2x128 colour 2x64': '0010001',
    'foc sigma 2x128 colour 2x128': '0000001',
    'foc sigma 2x128 colour 3x64': '0010001',
    'foc sigma 2x128 colour 3x128': '0000001',
    'foc sigma 2x128 colour 4x64': '0000001',
    'foc sigma 2x128 colour 4x128': '0000001',
    'foc sigma 3x32 colour 2x64': '1010001',
    'foc sigma 3x32 colour 2x128': '1000001',
    'foc sigma 3x32 colour 3x64': '1010001',
    'foc sigma 3x32 colour 3x128': '1000001',
    'foc sigma 3x32 colour 4x64': '1000001',
    'foc sigma 3x32 colour 4x128': '1000001',
    'foc sigma 3x64 colour 2x64': '1010001',
    'foc sigma 3x64 colour 2x128': '1000001',
    'foc sigma 3x64 colour 3x64': '1111001',
    'foc sigma 3x64 colour 3x128': '1000001',
    'foc sigma 3x64 colour 4x64': '1000001',
    'foc sigma 3x64 colour 4x128': '1000001',
    'foc sigma 3x128 colour 2x64': '0010001',
    'foc sigma 3x128 colour 2x128': '0000001',
    'foc sigma 3x128 colour 3x64': '0010001',
    'foc sigma 3x128 colour 3x128': '0000001',
    'foc sigma 3x128 colour 4x64': '0000001',
    'foc sigma 3x128 colour 4x128': '0000001',
    'foc sigma 4x32 colour 2x64': '1010001',
    'foc sigma 4x32 colour 2x128': '1000001',
    'foc sigma 4x32 colour 3x64': '1010001',
    'foc sigma 4x32 colour 3x128': '1000001',
    'foc sigma 4x32 colour 4x64': '1000001',
    'foc sigma 4x32 colour 4x128': '1000001',
    'foc sigma 4x64 colour 2x64': '1010001',
    'foc sigma 4x64 colour 2x128': '1000001',
    'foc sigma 4x64 colour 3x64': '1010001',
    'foc sigma 4x64 colour 3x128': '1000001',
    'foc sigma 4x64 colour 4x64': '1000001',
    'foc sigma 4x64 colour 4x128': '1000001',
    'foc sigma 4x128 colour 2x64': '0010001',
    'foc sigma 4x128 colour 2x128': '0000001',
    'foc sigma 4x128 colour 3x64': '0010001',
    'foc sigma 4x128 colour 3x128': '0000001',
    'foc sigma 4x128 colour 4x64': '0000001',
    'foc sigma 4x128 colour 4x128': '0000001',
    'foc encoder not a hash grid': '0010001',
    'foc encoder input_dim 2': '0010001',
    'foc encoder level_dim 4': '0010001',
    'foc encoder output 48 wide': '0010001',
    'foc gridtype tiled': '1111001',
    'foc align_corners': '1111001',
    'foc interpolation smoothstep': '1111001',
    'foc sigma_net not an FFMLP': '0010001',
    'foc sigma input 48': '1010001',
    'foc sigma input 80': '0010001',
    'foc sigma layers 5': '0010001',
    'foc sigma output 32 wide': '0010001',
    'foc sigma output activation relu': '1011001',
    'foc sigma activation sigmoid': '0010001',
    'foc sigma activation none': '1010001',
    'foc color_net not an FFMLP': '1000001',
    'foc colour input 64': '1000001',
    'foc colour output 32 wide': '1000001',
    'foc colour activation sigmoid': '1000001',
    'foc colour activation none': '1010001',
    'foc both activations none': '1110001',
    'foc encoder_dir not SH': '1000000',
    'foc SH degree 3': '1111001',
    'foc geo_feat_dim 14': '1000000',
    'foc yolo_encoding_dim 8': '1000000',
    'foc bg_radius 1': '1111001',
    'foc density_scale 2': '1111001',
    'foc FOC_FUSED_FIELD=0': '0010001',
    'foc FOC_FUSED_HEAD=0': '1111000',
    'foc FOC_FUSED_TAIL=0': '1001001',
    'foc FOC_FUSED_INFER=0': '1110001',
    'foc FOC_FUSED_OCC=0': '1111001',
    'foc FOC_RENDER_NATIVE=0': '1111001',
    'foc FOC_MLP_BWD_FUSED=0': '0010001',
    'foc FOC_FIELD_FWD_FUSED=0': '1011001',
}

# row -> (the plan's verdicts, why they differ from the old predicates'); SHEncoder refuses any degree but 4, and network_foc's constructor
# always builds two FFMLPs with a 48-wide colour input
PLAN_DIFFERS = {
    "ff SH degree 3": ("1000000", "the SH degree is checked once for every path that reads SH rows; only the head's check had it"),
    "foc SH degree 3": ("1000000", "the SH degree is checked once for every path that reads SH rows; FOC's head check lacked it"),
    "foc sigma_net not an FFMLP": ("0010000", "the head kernels need both networks to be FFMLPs; FOC's head check lacked it"),
    "foc color_net not an FFMLP": ("1000000", "the head kernels need both networks to be FFMLPs; FOC's head check lacked it"),
    "foc colour input 64": ("1000000", "the head kernels write the colour net's input rows (32 or 48 wide); FOC's head check lacked "
                            "the width, the ff network's read it from in_dim_color"),
}
