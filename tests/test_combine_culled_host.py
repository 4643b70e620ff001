"""CPU: the host side of the combine fed from culled lists (include/focnerf.h FocCulledField / foc_combine_select_composite_culled,
combine.combine_culled / culled_field_fns): the refusals that need no device, the argument checks."""
import ctypes

import pytest


def test_refusals_need_no_gpu():
    """Every refusal comes from the host, before any launch: made-up pointers are never dereferenced."""
    from focnerf_amd import _lib
    lib, S = _lib.lib, _lib.FocCulledField
    one = ctypes.c_void_p(64)
    bgs = (ctypes.c_float * 2)(1.0, 0.0)

    def call(K=2, struct_bytes=ctypes.sizeof(S), ids=None, n_obj=0, nears=one, fars=one, N=4, T=8, bgs=bgs, n_bg=2, image4=one, depth=one, att=(None, None, None),
             edit=None, objs=True):
        arr = (S * 17)()
        for o in arr:
            o.mask = o.offsets = o.sigma_c = o.rgb_c = 64
            o.m_occ, o.density_scale, o.thresh, o.sigma_gain = 3, 1.0, 1e-10, 1.0
        if edit:
            edit(arr[1])
        return lib.foc_combine_select_composite_culled(arr if objs else None, K, struct_bytes, ids, n_obj, nears, fars, N, T, bgs, n_bg, image4, depth, None,
                                                       att[0], att[1], att[2], None, None)

    def field(name, value):
        return lambda o: setattr(o, name, value)
    cases = [(dict(K=0), b"1 <= K <= 16"), (dict(K=17), b"1 <= K <= 16"), (dict(struct_bytes=44), b"bytes"), (dict(objs=False), b"objs is null"),
             (dict(nears=None), b"null pointer"), (dict(fars=None), b"null pointer"), (dict(image4=None), b"null pointer"), (dict(depth=None), b"null pointer"),
             (dict(edit=field("mask", None)), b"mask / offsets"), (dict(edit=field("offsets", None)), b"mask / offsets"),
             (dict(edit=field("sigma_c", None)), b"null sigma / rgb"), (dict(edit=field("rgb_c", None)), b"null sigma / rgb"),
             (dict(n_bg=0), b"one or two backgrounds"), (dict(n_bg=3), b"one or two backgrounds"), (dict(bgs=None), b"one or two backgrounds"),
             (dict(T=1), b"T must be >= 2"), (dict(N=1 << 22, T=512), b"2^31"),
             (dict(n_obj=4, ids=(ctypes.c_uint32 * 2)(0, 4), att=(one, one, one)), b"ids[1] = 4 is not below n_obj = 4"),
             (dict(n_obj=1, att=(one, one, one)), b"ids[1] = 1 is not below n_obj = 1"), (dict(n_obj=17, att=(one, one, one)), b"n_obj <= 16"),
             (dict(n_obj=4, att=(None, one, one)), b"must not be null"), (dict(n_obj=4, att=(one, None, one)), b"must not be null"),
             (dict(n_obj=4, att=(one, one, None)), b"must not be null"), (dict(edit=field("mask", 68)), b"aligned")]
    cases += [(dict(edit=field("sigma_gain", g)), b"sigma_gain must be finite and > 0") for g in (0.0, -2.0, float("nan"), float("inf"))]
    for kw, message in cases:
        assert call(**kw) == 1, kw
        err = lib.foc_last_error()
        assert err.startswith(b"combine_select_composite_culled:") and message in err, (kw, err)
    # no rays: nothing to launch, nothing to read
    assert call(N=0) == 0 and call(N=0, nears=None, fars=None, image4=None, depth=None) == 0


def test_combine_culled_checks_its_arguments():
    import torch
    from focnerf_amd.combine import combine_culled
    from focnerf_amd.fixedcull import CulledField
    z = torch.zeros(4)
    c = CulledField(None, None, 0, None, None, 1.0, 1e-10, 1.0, 4, 8)
    with pytest.raises(ValueError, match="1 to 16 objects"):
        combine_culled([], z, z)
    with pytest.raises(ValueError, match="1 to 16 objects"):
        combine_culled([c] * 17, z, z)
    with pytest.raises(ValueError, match="CulledField"):
        combine_culled([c, torch.zeros(4, 8, 4)], z, z)
    with pytest.raises(ValueError, match="one chunk, one T"):
        combine_culled([c, CulledField(None, None, 0, None, None, 1.0, 1e-10, 1.0, 4, 9)], z, z)
    with pytest.raises(ValueError, match="nears / fars"):
        combine_culled([c], torch.zeros(5), torch.zeros(5))


def test_culled_field_fns_checks_its_arguments_like_placed_field_fns():
    import torch
    from focnerf_amd import Placement
    from focnerf_amd.combine import culled_field_fns, placed_field_fns
    rays = torch.zeros(4, 3)
    box = torch.tensor([-2.0] * 3 + [2.0] * 3)
    for fn, who in ((culled_field_fns, "culled_field_fns"), (placed_field_fns, "placed_field_fns")):
        with pytest.raises(ValueError, match=who + ": 0 models"):
            fn([], [], [], rays, rays, 8, box)
        with pytest.raises(ValueError, match=who + ": 2 models, 1 occupancies"):
            fn([object(), object()], [None], [None, None], rays, rays, 8, box)
        with pytest.raises(ValueError, match=who + ": 1 models, 1 occupancies, 1 placements, 2 yolo_details"):
            fn([object()], [None], [Placement()], rays, rays, 8, box, yolo_details=[None, None])
