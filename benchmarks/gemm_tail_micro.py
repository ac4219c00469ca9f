"""The act16 dgrad and wgrad ops at the flagship shape with and without an m
tail, each call repeated between device events (profiles/18).

    python benchmarks/gemm_tail_micro.py [TAG] [TILE]

TILE forces the wgrad's output tile (1 / 2 / 3 = 128x128 / 256x128 / 256x256;
default 0, the dispatch's choice; profiles/21).

m = 1412 * 128 is tail-free for every tile; m + 26 leaves 26 rows past the
last 128-row (and 64-row) tile.  The dgrad figure includes the transposed
weight-image kernel (no saved image is passed).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pertgnn._C as C  # noqa: E402

N, K = 1024, 256
M_FULL = 1412 * 128
M_TAIL = M_FULL + 26


def timeit(f, iters=200, warm=30):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "tree"
    tile = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
    gy_all = torch.randn(M_TAIL, N, device=dev).to(torch.bfloat16)
    x_all = torch.randn(M_TAIL, K, device=dev).to(torch.bfloat16)
    for rep in range(2):
        for m in (M_FULL, M_TAIL):
            gy, x = gy_all[:m], x_all[:m]
            t_d = timeit(lambda: C.linear_dgrad16_o16(gy, w))
            t_w = timeit(lambda: C.linear_wgrad16_b16(gy, x, True, tile=tile))
            print(f"{tag} rep{rep} m={m}: dgrad op {t_d:.2f} us  "
                  f"wgrad op {t_w:.2f} us", flush=True)


if __name__ == "__main__":
    main()
