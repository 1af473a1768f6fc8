"""The group route of attn_bwd's dK/dV under GQA (attention.hip:
attn_bwd_kernel<..., GROUP>, dkv_route=1): one block per 64 keys of a KV head
loops over the q heads of the group and stores bf16 once; no atomics.

Reference, floor and criterion are tests/attn_ref.py's.  Every call names its
route, so nothing here depends on what attn_bwd's auto mode takes, except the
last assertion of test_reproducible_and_routes_agree (see there).

The refusals under SAMD_ATTN_BWD_TR16=0 / SAMD_ATTN_BWD_VL2=1 are not run:
the switches are read once per process and the children of attn_run.run_child
do fixed work that never passes dkv_route.  They are two TORCH_CHECKs on
group_route_refusal(), beside the dkv_route range check tested below.
"""

import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402  (plain helper modules beside this file)
import attn_run as run  # noqa: E402

pytestmark = pytest.mark.gpu
GQA = [(2, 6, 2), (3, 4, 1)]       # G = 3; MQA with an odd B * Hkv


@run.launch_guard
def _direct(q, k, v, causal, do, route, *, lo=None, p=0.0, seed=0):
    """run.kernel_direct with attn_bwd's dkv_route: (out, lse, dq, dk, dv)."""
    from saturn_amd.ops.flash import _pad_t64

    T = q.shape[2]
    qp, kp, vp, dop = (_pad_t64(t) for t in (q, k, v, do))
    if lo is not None:
        lo = torch.nn.functional.pad(lo, (0, (-T) % 64), value=T - 1).contiguous()
    kw = run._set(p, seed, kv_lo=lo)
    o, lse = run.ext().attn_fwd(qp, kp, vp, causal, T, **kw)
    dq, dk, dv = run.ext().attn_bwd(dop, qp, kp, vp, o, lse, causal, T,
                                    dkv_route=route, **kw)
    return tuple(t[:, :, :T] for t in (o, lse, dq, dk, dv))


def _check(name, c, got):
    rep, bad = ar.check_case(got, c["ref"], c["base"], c["lse_tol"])
    print("ATTN_RATIO", "gqa-group", name, json.dumps(ar.ratios(rep)))
    assert not bad, bad


def _same(a, b, names, why):
    for n in names:
        i = ar.NAMES.index(n)
        assert run.bits_equal(a[i], b[i]), f"{n}: {why}"


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [128, 192])      # v2 and v1 forward; 2, 3 blocks
@pytest.mark.parametrize("B,H,Hkv", GQA)
@pytest.mark.parametrize("D", ar.DS)
def test_numerics(D, B, H, Hkv, T, causal):
    c = ar.case("randn", B, H, Hkv, T, D, causal)
    args, kw = run.on_device(c)
    _check(f"D{D}-B{B}H{H}kv{Hkv}-T{T}-{'c' if causal else 'n'}", c,
           _direct(*args, 1, **kw))


@pytest.mark.parametrize("D", [64, 256])
def test_one_head_group_is_the_plain_kernel(D):
    """Hkv == H: G = 1, the accumulation order of the plain kernel."""
    args = ar.make_inputs("randn", 2, 3, 3, 192, D, "cuda", seed=31)
    q, k, v, do = args
    _same(_direct(q, k, v, True, do, 1), _direct(q, k, v, True, do, 0),
          ("dk", "dv"), "G = 1 differs from the plain kernel")


@pytest.mark.parametrize("g", [0, 1, 2])
def test_head_map(g):
    """dO = 0 on all q heads but h_kv * 3 + g: the other heads add exact
    zeros, so dk/dv are the bits of an MHA call on those q heads alone."""
    q, k, v, do = ar.make_inputs("randn", 2, 6, 2, 192, 128, "cuda", seed=32)
    sel = [g, 3 + g]
    do_z = torch.zeros_like(do)
    do_z[:, sel] = do[:, sel]
    got = _direct(q, k, v, True, do_z, 1)
    want = _direct(q[:, sel].contiguous(), k, v, True, do[:, sel].contiguous(), 0)
    _same(got, want, ("dk", "dv"), f"group route, head {g} of each group")


@pytest.mark.parametrize("bound", ["W65_T256", "docs_T256"])
@pytest.mark.parametrize("D", [128, 256])
def test_kv_lo(D, bound):
    """The early break of a head's q loop must not end the head loop."""
    c = ar.case("randn", 2, 8, 2, 256, D, bound=bound)
    args, kw = run.on_device(c)
    _check(f"D{D}-{bound}", c, _direct(*args, 1, **kw))
    out, dq, dk, dv = run.kernel_public(*args, lo=kw["lo"])
    _check(f"D{D}-{bound}-public", c, (out, None, dq, dk, dv))


@pytest.mark.parametrize("D", [64, 256])
def test_dropout(D):
    """The mask counter takes the q head: a kv-head counter fails dk and dv."""
    c = ar.case("randn", 2, 6, 2, 192, D, p=0.1, seed=ar.DROP_INPUT_SEED)
    args, kw = run.on_device(c)
    _check(f"D{D}-p0.1", c, _direct(*args, 1, **kw))


def test_reproducible_and_routes_agree():
    """Two group calls give the same bits; dq does not depend on the route.
    Direct calls only (ragged T = 130, padded to 192): attn_bwd's auto mode
    takes the group route from 768 blocks (B * Hkv * T/64) and this call has
    12, so the public wrapper stays on the atomic route here and its dk/dv
    are not comparable bit for bit."""
    q, k, v, do = ar.make_inputs("randn", 2, 6, 2, 130, 128, "cuda", seed=33)
    a, b = _direct(q, k, v, True, do, 1), _direct(q, k, v, True, do, 1)
    _same(a, b, ("dq", "dk", "dv"), "two group-route calls differ")
    _same(a, _direct(q, k, v, True, do, 0), ("dq",), "dq depends on dkv_route")


@pytest.mark.parametrize("D", ar.DS)
def test_dispatch_and_refusals(D):
    tr = 1 if D <= 128 else 0          # T = 192: the v1 forward at every D
    disp = run.ext().attn_dispatch
    for flags, tail in (({}, ""), ({"has_lo": True}, ",1"),
                        ({"has_drop": True}, ",0,1")):
        bwd = f"{D},{tr},0" + (tail + ",0,0,0")[:6] + ",1"
        assert disp(192, D, gqa=True, **flags) == (
            f"attn_fwd_kernel<{D}{tail}> attn_delta_kernel<{D}> "
            f"attn_bwd_kernel<{bwd}> attn_dq_kernel<{D},{tr},0{tail}>")
    with pytest.raises(RuntimeError, match="Hkv == H"):
        disp(192, D, ds_route=True, gqa=True)
    q, k, v, do = ar.make_inputs("randn", 1, 2, 1, 64, D, "cuda", seed=34)
    o, lse = run.ext().attn_fwd(q, k, v, True, 64)
    with pytest.raises(RuntimeError, match="attn_bwd: dkv_route must be"):
        run.ext().attn_bwd(do, q, k, v, o, lse, True, 64, dkv_route=2)
