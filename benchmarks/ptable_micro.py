"""Microbench of the P-table GEMMs at the flagship table shapes (V=2048
interfaces, R=5 rpc types, H=256; L = 8 and 16 layers): the per-layer calls
(``linear16`` forward; ``linear_dgrad16`` + ``linear_wgrad16`` and the adds
of the per-layer table gradients in the backward) against the grouped
``ptables_fwd`` / ``ptables_bwd``, over the dgrad's layer split.

Every variant is captured into a hipGraph of REPS back-to-back calls and the
replay is timed, as the training step runs them: eager timing of 4-32-block
kernels measures the host's launch rate, not the GPU.  Operands stay
L2/Infinity-Cache resident between calls here, as they mostly do in the step
(tables and weights are 2 MB + 0.25 MB per layer).

Run (GPU box): PYTHONPATH=. python benchmarks/ptable_micro.py
"""
import time

import torch

REPS = 20


def graph_us(fn, replays=20):
    """µs per call of fn inside a captured graph of REPS calls."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(REPS)]
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    del keep
    return (time.perf_counter() - t0) / (replays * REPS) * 1e6


def main():
    import pertgnn._C as C

    dev = torch.device("cuda:0")
    V, R, h = 2048, 5, 256
    gen = torch.Generator().manual_seed(0)
    ifc = torch.randn(V, h, generator=gen).to(dev)
    rpc = torch.randn(R, h, generator=gen).to(dev)
    none = torch.empty(0, device=dev)
    for layers in (8, 16):
        we_ifc = [(torch.randn(h, h, generator=gen) / 16).to(dev)
                  for _ in range(layers)]
        we_rpc = [(torch.randn(h, h, generator=gen) / 16).to(dev)
                  for _ in range(layers)]
        dps = [torch.randn(rows, h, generator=gen).to(torch.bfloat16).to(dev)
               for rows in [V] * layers + [R] * layers]

        def fwd_old():
            return ([C.linear_fwd_bf16_o16(ifc, w, none) for w in we_ifc]
                    + [C.linear_fwd_bf16_o16(rpc, w, none) for w in we_rpc])

        def fwd_new():
            return C.ptables_fwd(ifc, rpc, we_ifc, we_rpc)

        def bwd_old():
            out = []
            for t, (table, ws) in enumerate(((ifc, we_ifc), (rpc, we_rpc))):
                dt = None
                for l in reversed(range(layers)):
                    d = dps[t * layers + l]
                    g = C.linear_dgrad16(d, ws[l])
                    out.append(C.linear_wgrad16(d, table, False)[0])
                    dt = g if dt is None else dt + g
                out.append(dt)
            return out

        for a, b in zip(fwd_old(), fwd_new()):
            assert torch.equal(a, b)
        print(f"L={layers:<2} forward  per-layer ({2 * layers} launches) "
              f"{graph_us(fwd_old):7.1f} us   grouped {graph_us(fwd_new):6.1f} us")
        print(f"L={layers:<2} backward per-layer (dgrad, wgrad, memset, adds) "
              f"{graph_us(bwd_old):7.1f} us")
        for splits in (1, 2, 4, layers):
            fn = lambda: C.ptables_bwd(dps, ifc, rpc, we_ifc, we_rpc, splits)
            print(f"L={layers:<2} backward grouped, dgrad split {splits:<2}"
                  f"{graph_us(fn):28.1f} us")


if __name__ == "__main__":
    main()
