"""Microbench of the edge-table gradient at the flagship shape (E=237k edges
x h=256 bf16 de, V=2048 interfaces, R=5 rpc types, half the edges on
interface 0): the two per-table scatters plus the two bf16 casts against
the single-pass ``edge_table_grad``, back to back, over the chunk size C
(``PERTGNN_SCATTER_ITERS``) and the rows in flight per wave U.

The TB/s column is the 121 MB of de over the wall time of the whole entry
point (partials and tables are a few MB on top).  Back-to-back calls reuse
the same de, so part of it is served from the Infinity Cache: the numbers
rank the variants, the kernel trace of bench.py gives the in-step times.

Run (GPU box): PYTHONPATH=. python benchmarks/edge_table_micro.py
"""
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


def main():
    import pertgnn._C as C
    from pertgnn.ops import functional as F

    dev = torch.device("cuda:0")
    E, V, R, h = 237_000, 2048, 5, 256
    g = torch.Generator().manual_seed(0)
    ifc = torch.randint(0, V, (E,), generator=g)
    ifc[torch.randperm(E, generator=g)[: E // 2]] = 0
    rpc = torch.randint(0, R, (E,), generator=g)
    ea = torch.stack([ifc, rpc, torch.ones(E, dtype=torch.long),
                      torch.zeros(E, dtype=torch.long)], dim=1).to(dev)
    de = torch.randn(E, h, generator=g).to(torch.bfloat16).to(dev)
    nbytes = E * h * 2

    def old():
        dp = F._table_grad(C, de, ea[:, 0], V, h, 0).to(torch.bfloat16)
        dr = F._table_grad(C, de, ea[:, 1], R, h, 0).to(torch.bfloat16)
        return dp, dr

    old_p, old_r = old()
    us = timeit(old)
    print(f"two _table_grad + casts            {us:7.1f} us  "
          f"{nbytes / us / 1e6:4.2f} TB/s (of one de read)")
    want = torch.zeros(V + R, h, device=dev)
    want[:V].index_add_(0, ea[:, 0], de.float())
    want[V:].index_add_(0, ea[:, 1], de.float())
    for c in (32, 64, 128):
        plan = F.edge_table_plan(ea, V, R, C=c)
        lens3 = plan.lptr3[1:] - plan.lptr3[:-1]
        for u in (4, 8):
            fn = lambda: C.edge_table_grad(de, *plan.tensors(), V, R,
                                           torch.bfloat16, unroll=u)
            us = timeit(fn)
            err = float((fn().float() - want).abs().max())
            print(f"edge_table_grad C={c:<3} U={u} n1={plan.n1:<6} "
                  f"n2={plan.n2:<4} max|L3|={int(lens3.max()):<3} "
                  f"{us:7.1f} us  {nbytes / us / 1e6:4.2f} TB/s  "
                  f"max err vs fp32 index_add {err:.2e} "
                  f"(old path {float((torch.cat([old_p, old_r]).float() - want).abs().max()):.2e})")


if __name__ == "__main__":
    main()
