"""Time swiglu_bwd_t (llama_mlp_bwd.hip) against the kernels it replaces.

    python tools/llama_mlp_bwd_bench.py [M F]        default 8192 14336

Arms, alternating in one process, 10 windows of 5 calls each ending in a
synchronise, median [min..max] us:

    replaced      swiglu_bwd + d_gate.t().contiguous() + d_up.t().contiguous()
                  + swiglu_fwd: what the TN route would need without the kernel
    swiglu_bwd_t  both flags on
    copy          a bf16 copy of 4 [M, F] tensors' worth (8 B per element
                  read + 8 B written): the bandwidth for the traffic floor

swiglu_bwd_t moves 16 B per element (three reads, five writes of 2 B); its
floor is that over the copy's measured bandwidth.  Rule: swiglu_bwd_t's median
must not exceed the replaced sum's median plus that sum's own min..max spread.
Also prints the one-flag and no-flag instantiations.
"""

from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from wgrad_layout_probe import fmt, window_arms  # noqa: E402


def main() -> None:
    import torch

    from saturn_amd.ops import require_ext

    ext = require_ext()
    M, F = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (8192, 14336)
    torch.manual_seed(0)
    gate = (2 * torch.randn(M, F, device="cuda")).bfloat16()
    up = torch.randn(M, F, device="cuda").bfloat16()
    d_act = torch.randn(M, F, device="cuda").bfloat16()
    src = torch.empty(4, M, F, device="cuda", dtype=torch.bfloat16).normal_()
    dst = torch.empty_like(src)

    def replaced():
        dg, du = ext.swiglu_bwd(d_act, gate, up)
        dg.t().contiguous()
        du.t().contiguous()
        ext.swiglu_fwd(gate, up)

    r = window_arms({
        "replaced": replaced,
        "swiglu_bwd_t": lambda: ext.swiglu_bwd_t(d_act, gate, up, True, True),
        "copy": lambda: dst.copy_(src),
        "swiglu_bwd_t gu=1 down=0": lambda: ext.swiglu_bwd_t(d_act, gate, up, True, False),
        "swiglu_bwd_t gu=0 down=1": lambda: ext.swiglu_bwd_t(d_act, gate, up, False, True),
        "swiglu_bwd_t gu=0 down=0": lambda: ext.swiglu_bwd_t(d_act, gate, up, False, False),
        "swiglu_bwd alone": lambda: ext.swiglu_bwd(d_act, gate, up),
    })
    print(f"M={M} F={F} bf16, 10 windows x 5 calls, median [min..max] us")
    for name, row in r.items():
        print(f"  {name:26s} {fmt(row)}")
    traffic = 16.0 * M * F
    bw = traffic / r["copy"][0] / 1e6  # the copy moves 16 B per element too
    new, old = r["swiglu_bwd_t"], r["replaced"]
    print(f"  copy bandwidth {bw:.2f} TB/s; traffic floor of swiglu_bwd_t "
          f"({traffic / 1e9:.2f} GB) {r['copy'][0]:.1f} us; swiglu_bwd_t is "
          f"x{new[0] / r['copy'][0]:.2f} of it ({traffic / new[0] / 1e6:.2f} TB/s)")
    limit = old[0] + (old[2] - old[1])
    print(f"  swiglu_bwd_t / replaced x{new[0] / old[0]:.3f}; limit "
          f"{limit:.1f} us; no slower: {new[0] <= limit}")


if __name__ == "__main__":
    main()
