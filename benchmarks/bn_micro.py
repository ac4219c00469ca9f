"""Microbench of the BN channel-reduction kernels at the flagship shape
(n=180780 rows x h=256, bf16 streams) across PERTGNN_BN_BLOCKS settings.

Times the three y-taking entry points, their keep-mask variants, the forward
apply that writes the mask, and both cross-block combine candidates
(PERTGNN_BN_COMBINE=slab|atomic).  The TB/s column is bytes actually moved
by the call's big streams (printed next to it) over the wall time of the
whole entry point, small fold/finalize launches included.

Run (GPU box): for B in 512 1024 2048 2825; do
  PERTGNN_BN_BLOCKS=$B PYTHONPATH=. python benchmarks/bn_micro.py; done
"""
import os
import time

import torch


def timeit(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def line(name, us, nbytes):
    print(f"  {name:<34} {us:7.1f} us  {nbytes / 1e6:6.1f} MB  "
          f"{nbytes / us / 1e6:4.1f} TB/s")


def main():
    import pertgnn._C as C

    dev = torch.device("cuda:0")
    n, h = 180780, 256
    x = torch.randn(n, h, device=dev).to(torch.bfloat16)
    g = torch.randn(n, h, device=dev).to(torch.bfloat16)
    gamma = torch.ones(h, device=dev)
    beta = torch.zeros(h, device=dev)
    rm = torch.zeros(h, device=dev)
    rv = torch.ones(h, device=dev)
    seed = torch.empty(0, dtype=torch.int64, device=dev)
    out = C.bn_relu_fwd16(x, gamma, beta, rm, rv, 0.1, 1e-5, True, True, 0.0,
                          seed)
    y, mean, invstd = out[:3]
    mask = out[3] if len(out) > 3 and out[3].numel() else None

    s = n * h * 2  # one bf16 stream
    mb = n * h // 8  # the bit-packed mask
    blocks = os.environ.get("PERTGNN_BN_BLOCKS", "512(default)")
    for combine in ("slab", "atomic"):
        os.environ["PERTGNN_BN_COMBINE"] = combine
        print(f"blocks={blocks} combine={combine}")
        line("bn_stats", timeit(lambda: C.bn_stats(x)), s)
        line("bn_bwd_partials16 (y)", timeit(
            lambda: C.bn_bwd_partials16(g, x, y, mean, invstd, True, 1.0)),
            3 * s)
        part = C.bn_bwd_partials16(g, x, y, mean, invstd, True, 1.0)
        if mask is not None:
            line("bn_bwd_partials16 (mask)", timeit(
                lambda: C.bn_bwd_partials16(g, x, mask, mean, invstd, True,
                                            1.0)), 2 * s + mb)
            line("bn_relu_bwd16 (mask, whole bwd)", timeit(
                lambda: C.bn_relu_bwd16(g, x, gamma, mean, invstd, mask, True,
                                        1.0)), 5 * s + 2 * mb)
        line("bn_relu_bwd16 (y, whole bwd)", timeit(
            lambda: C.bn_relu_bwd16(g, x, gamma, mean, invstd, y, True, 1.0)),
            7 * s)
        line("bn_relu_fwd16 (whole fwd)", timeit(
            lambda: C.bn_relu_fwd16(x, gamma, beta, rm, rv, 0.1, 1e-5, True,
                                    True, 0.0, seed)),
            3 * s + (mb if mask is not None else 0))
    os.environ.pop("PERTGNN_BN_COMBINE")
    # the apply kernels do not depend on the combine
    line("bn_bwd_apply16 (y)", timeit(
        lambda: C.bn_bwd_apply16(g, x, y, mean, invstd, gamma, part, part,
                                 True, 1.0)), 4 * s)
    if mask is not None:
        line("bn_bwd_apply16 (mask)", timeit(
            lambda: C.bn_bwd_apply16(g, x, mask, mean, invstd, gamma, part,
                                     part, True, 1.0)), 3 * s + mb)

    # parity across block counts (vs plain torch fp32 on rounded operands)
    p = C.bn_stats(x)
    xs = x.float()
    ref_s = xs.sum(0)
    ref_q = (xs * xs).sum(0)
    rel = max((p[:h] - ref_s).abs().max().item() / ref_s.abs().max().item(),
              (p[h:2 * h] - ref_q).abs().max().item() / ref_q.abs().max().item())
    assert p[2 * h].item() == n
    print(f"  stats relerr vs fp32: {rel:.2e}")


if __name__ == "__main__":
    main()
