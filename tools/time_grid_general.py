"""tools/time_grid_general.py LIB_A LIB_B [--rounds N]: the grid encoder's general kernels (not the fp16 D = 3 C = 2 training path, which
bench.py covers) under two builds of the library, in ms per call at 2^18 random points. Each round starts one fresh process per library
(FOCNERF_LIB_PATH), A then B; a process warms up every case and times 20 calls of it between device events. Prints per case the median
over the rounds for A and B, their ratio, and the spread (max / min over the rounds) of each — give the same build twice to see the
scatter of the method. Without arguments: times the library of this checkout once and prints {case: ms}."""
import json
import os
import statistics
import subprocess
import sys

B, CALLS = 1 << 18, 20


def cases():
    import numpy as np
    import torch
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from focnerf_amd.gridencoder import level_offsets

    def run(fn, *args):
        check(fn(*args, stream_of(None)), fn.__name__)

    def timed(f):
        for _ in range(3):
            f()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS):
            f()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / CALLS

    out = {}
    # (name, D, C, L, H, log2_hash, per-level scale, dtype, dy_dx): the background encoder's shape, the D = 3 general path, D = 4 / 5
    shapes = [("bg D=2 f16", 2, 2, 16, 16, 19, 1.3819, torch.float16, False), ("D=3 f16 dy_dx", 3, 2, 16, 16, 19, 1.3819, torch.float16, True),
              ("D=3 f32", 3, 2, 16, 16, 19, 1.3819, torch.float32, False), ("D=3 f32 dy_dx", 3, 2, 16, 16, 19, 1.3819, torch.float32, True),
              ("D=3 f32 C=4", 3, 4, 16, 16, 19, 1.3819, torch.float32, False), ("D=3 f32 C=4 dy_dx", 3, 4, 16, 16, 19, 1.3819, torch.float32, True),
              ("D=4 f16", 4, 2, 8, 8, 16, 1.5, torch.float16, True), ("D=5 f32", 5, 2, 8, 4, 16, 1.5, torch.float32, True)]
    for name, D, C, L, H, lh, pls, tdt, with_dy in shapes:
        g = torch.Generator().manual_seed(D)
        code, S = int(tdt == torch.float16), float(np.log2(pls))
        off = torch.from_numpy(level_offsets(D, L, pls, H, lh)).cuda()
        rows = int(off[-1])
        x = torch.rand(B, D, generator=g).cuda()
        table = (torch.rand(rows, C, generator=g) - 0.5).cuda().to(tdt)
        grad = (torch.randn(L, B, C, generator=g) * 0.1).cuda().to(tdt)
        outp, ge = torch.empty(L, B, C, dtype=tdt, device="cuda"), torch.zeros(rows, C, dtype=tdt, device="cuda")
        dy = torch.empty(B, L * D * C, dtype=tdt, device="cuda") if with_dy else None
        gi = torch.empty(B, D, dtype=tdt, device="cuda") if with_dy else None
        fwd = (ptr(x), ptr(table), ptr(off), ptr(outp), B, D, C, L, S, H, ptr(dy), 0, 0, 0, code, None)
        out[name + " forward"] = timed(lambda: run(lib.foc_grid_encode_forward, *fwd))
        out[name + " forward_bl"] = timed(lambda: run(lib.foc_grid_encode_forward_bl, *fwd))
        out[name + " backward"] = timed(lambda: run(lib.foc_grid_encode_backward, ptr(grad), ptr(x), ptr(table), ptr(off), ptr(ge), B, D, C, L, S, H, ptr(dy), ptr(gi),
                                                    0, 0, 0, code, 0, None))
        if D >= 4:
            out[name + " grad_tv"] = timed(lambda: run(lib.foc_grad_total_variation, ptr(x.to(tdt)), ptr(table), ptr(ge), ptr(off), 1e-7, B, D, C, L, S, H, 0, 0, code))
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    args, rounds = sys.argv[1:], 5
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i: i + 2]
    if not args:
        print(json.dumps(cases()))
        return
    if len(args) != 2:
        sys.exit("usage: time_grid_general.py [LIB_A LIB_B [--rounds N]]")
    got = {0: [], 1: []}
    for _ in range(rounds):
        for i, path in enumerate(args):
            env = dict(os.environ, FOCNERF_LIB_PATH=os.path.abspath(path))
            got[i].append(json.loads(subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True, text=True,
                                                    timeout=300).stdout.strip().splitlines()[-1]))
    print(f"{'case':28s} {'A ms':>8s} {'B ms':>8s} {'B/A':>6s} {'A max/min':>9s} {'B max/min':>9s}")
    for name in got[0][0]:
        a, b = [r[name] for r in got[0]], [r[name] for r in got[1]]
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"{name:28s} {ma:8.4f} {mb:8.4f} {mb / ma:6.3f} {max(a) / min(a):9.3f} {max(b) / min(b):9.3f}")


if __name__ == "__main__":
    main()
