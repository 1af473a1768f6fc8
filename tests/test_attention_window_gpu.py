"""Attention with a per-row lower key bound (kv_lo: sliding windows, packed
documents) on the GPU: attention.hip's LO instantiations through ext.attn_fwd
/ ext.attn_bwd and saturn_amd.ops.flash, against the fp64 reference of
tests/attn_window_ref.py under attn_ref's `close` criterion, plus the exact
bitwise properties a correct mask and a correct tile skip must have.

Every shape has B*H <= 16 and T <= 384.  Each comparison prints an
``ATTN_RATIO window-<group> <case> <json>`` line (kernel error over the error
floor, per tensor); docs/kernels.md tabulates the worst per group.
"""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import attn_window_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DS = list(wr.DS)


def _ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def _lo_paths(T, D):
    """What attn_dispatch(has_lo=True) must report with no switch set."""
    fwd = "attn_fwd_v2_kernel" if (T % 128 == 0 and D <= 128) else "attn_fwd_kernel"
    tr = 1 if D <= 128 else 0
    return (f"{fwd}<{D},1> attn_delta_kernel<{D}> "
            f"attn_bwd_kernel<{D},{tr},0,1> attn_dq_kernel<{D},{tr},0,1>")


def _check(group, name, c, gqa=False):
    """Both routes for a case; they must agree bit for bit (dk/dv under GQA
    excepted: fp32 atomics in arrival order); the direct five are checked."""
    direct, public = wr.run_case(c, DEV)
    assert wr.bits_equal(public[0], direct[0]), "out: routes differ"
    assert wr.bits_equal(public[1], direct[2]), "dq: routes differ"
    if not gqa:
        assert wr.bits_equal(public[2], direct[3]), "dk: routes differ"
        assert wr.bits_equal(public[3], direct[4]), "dv: routes differ"
    routes = [direct]
    if gqa:
        routes.append((public[0], direct[1]) + public[1:])
    for got in routes:
        rep, bad = wr.check_case_lo(got, c["ref"], c["base"], c["lse_tol"])
        print("ATTN_RATIO", f"window-{group}", name, json.dumps(ar.ratios(rep)),
              "lse", json.dumps(rep.get("lse")))
        assert not bad, bad
    return direct


def _dev(c):
    return tuple(c[n].to(DEV) for n in ("q", "k", "v", "do", "lo"))


# ---------------------------------------------------------------------------
# A. the matrix: D x bound x input kind
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,bound,kind", wr.MATRIX,
                         ids=[f"D{d}-{b}-{k}" for d, b, k in wr.MATRIX])
def test_matrix(D, bound, kind):
    T = wr.BOUNDS[bound][0]
    path = _ext().attn_dispatch(T, D, has_lo=True)
    assert path == _lo_paths(T, D)
    # T=192 and T=320 reach v1; T=256 and T=384 reach v2 at D <= 128
    v2 = T in (256, 384) and D <= 128
    assert path.startswith(f"attn_fwd_v2_kernel<{D},1>" if v2
                           else f"attn_fwd_kernel<{D},1>")
    # without the keyword the report is the plain one
    assert ",1>" not in _ext().attn_dispatch(T, D).split()[0]
    c = wr.case(kind, *wr.BH, wr.BH[1], T, D, bound)
    _check("A", f"D{D}-{bound}-{kind}", c)


# ---------------------------------------------------------------------------
# B. a zero bound is the plain kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [192, 256])
@pytest.mark.parametrize("D", DS)
def test_zero_bound_is_the_plain_kernel(D, T):
    q, k, v, do = ar.make_inputs("randn", 2, 3, 3, T, D, DEV, seed=1)
    plain = ar.ext_fwd_bwd(q, k, v, True, do, T)
    for lo in (torch.zeros(T, dtype=torch.int32, device=DEV),
               torch.zeros(2, T, dtype=torch.int32, device=DEV)):
        got = wr.kernel_direct_lo(q, k, v, do, lo)
        for name, a, b in zip(ar.NAMES, got, plain):
            assert wr.bits_equal(a, b), name
    ref = ar.kernel_public(q, k, v, True, do)
    for W in (T, T + 5):
        got = wr.kernel_public_lo(q, k, v, do, window=W)
        for a, b in zip(got, ref):
            assert wr.bits_equal(a, b), W


# ---------------------------------------------------------------------------
# C. locality, bitwise
# ---------------------------------------------------------------------------
def _other(t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t.shape, generator=g).bfloat16().to(t.device)


@pytest.mark.parametrize("D", DS)
def test_window_locality_bitwise(D):
    T, W, j0, t0 = 256, 40, 100, 150
    q, k, v, do = ar.make_inputs("randn", 1, 3, 3, T, D, DEV, seed=3)
    lo = wr.window_bound(T, W).to(DEV)
    a = wr.kernel_direct_lo(q, k, v, do, lo)
    # keys below j0 replaced: rows t >= j0 + W - 1 never saw them
    k2, v2 = k.clone(), v.clone()
    k2[:, :, :j0] = _other(k[:, :, :j0], 1)
    v2[:, :, :j0] = _other(v[:, :, :j0], 2)
    b = wr.kernel_direct_lo(q, k2, v2, do, lo)
    r0 = j0 + W - 1
    for i in (0, 1, 2):                                   # out, lse, dq
        assert wr.bits_equal(a[i][:, :, r0:], b[i][:, :, r0:]), ar.NAMES[i]
        assert not wr.bits_equal(a[i][:, :, :r0], b[i][:, :, :r0])
    # rows from t0 replaced: keys j <= t0 - W are seen by earlier rows only
    q2, do2 = q.clone(), do.clone()
    q2[:, :, t0:] = _other(q[:, :, t0:], 3)
    do2[:, :, t0:] = _other(do[:, :, t0:], 4)
    b = wr.kernel_direct_lo(q2, k, v, do2, lo)
    j1 = t0 - W + 1
    for i in (3, 4):                                      # dk, dv
        assert wr.bits_equal(a[i][:, :, :j1], b[i][:, :, :j1]), ar.NAMES[i]
        assert not wr.bits_equal(a[i][:, :, j1:], b[i][:, :, j1:])


@pytest.mark.parametrize("D", DS)
def test_document_locality_bitwise(D):
    T, docs = 256, [70, 1, 129, 56]
    s3, e3 = 71, 200                                      # document 3
    q, k, v, do = ar.make_inputs("randn", 1, 3, 3, T, D, DEV, seed=4)
    lo = wr.docs_bound([docs], T).to(DEV)
    a = wr.kernel_direct_lo(q, k, v, do, lo)
    inside = [t.clone() for t in (q, k, v, do)]
    for i, t in enumerate(inside):
        t[:, :, s3:e3] = _other(t[:, :, s3:e3], 10 + i)
    b = wr.kernel_direct_lo(*inside, lo)
    for i, name in enumerate(ar.NAMES):
        assert wr.bits_equal(a[i][:, :, :s3], b[i][:, :, :s3]), name
        assert wr.bits_equal(a[i][:, :, e3:], b[i][:, :, e3:]), name
        assert not wr.bits_equal(a[i][:, :, s3:e3], b[i][:, :, s3:e3])
    # no other document contributes to document 3's dk / dv
    do0 = do.clone()
    do0[:, :, s3:e3] = 0
    z = wr.kernel_direct_lo(q, k, v, do0, lo)
    assert (z[3][:, :, s3:e3].float() == 0).all()
    assert (z[4][:, :, s3:e3].float() == 0).all()
    assert (z[3][:, :, e3:].float() != 0).any()


# ---------------------------------------------------------------------------
# D. W = 1: every row sees itself only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [192, 256])
@pytest.mark.parametrize("D", DS)
def test_window_of_one(D, T):
    c = wr.case("randn", 1, 3, 3, T, D, ("window", 1), seed=5)
    q, k, v, do, lo = _dev(c)
    out, lse, dq, dk, dv = wr.kernel_direct_lo(q, k, v, do, lo)
    assert wr.bits_equal(out, v) and wr.bits_equal(dv, do)   # p = 1 exactly
    diag = (q.double() * k.double()).sum(-1) / math.sqrt(D)   # the one score
    assert ar.max_err(c["ref"][1], diag.cpu()) < 1e-12
    err = ar.max_err(lse, diag)
    print("ATTN_RATIO window-D", f"D{D}T{T}", "lse",
          json.dumps({"err": err, "tol": c["lse_tol"]}))
    assert lse.dtype == torch.float32 and err <= c["lse_tol"]
    # dq and dk are exactly 0; the kernel returns the fp32 difference of two
    # D-term sums of the same products do_i * v_i (the dP MFMA and the delta
    # kernel): the T = 1 exception of docs/kernels.md, row by row
    ds = (2 * D * 2.0 ** -24 / math.sqrt(D)
          * (do.double() * v.double()).abs().sum(-1).max().item())
    assert torch.isfinite(dq.float()).all() and torch.isfinite(dk.float()).all()
    assert dq.abs().max().item() <= 1.02 * ds * k.abs().max().item()
    assert dk.abs().max().item() <= 1.02 * ds * q.abs().max().item()


# ---------------------------------------------------------------------------
# E. tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 31, 32, 33, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("D", [128, 256])
def test_window_tile_edges(D, W):
    T = 256
    path = _ext().attn_dispatch(T, D, has_lo=True)
    assert path.startswith("attn_fwd_v2_kernel<128,1>" if D == 128
                           else "attn_fwd_kernel<256,1>")
    c = wr.case("randn", 1, 3, 3, T, D, ("window", W), seed=6)
    _check("E", f"D{D}W{W}", c)


# ---------------------------------------------------------------------------
# F. ragged T through the public API
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,bound", [(130, ("window", 50)),
                                     (197, ("window", 50)),
                                     (197, ("docs", ((100, 97), (100, 97))))],
                         ids=["T130W50", "T197W50", "T197docs"])
@pytest.mark.parametrize("D", DS)
def test_ragged_T(D, T, bound):
    from saturn_amd.ops.flash import document_lo

    c = wr.case("randn", 2, 3, 3, T, D, bound, seed=7)
    q, k, v, do, lo = _dev(c)
    if bound[0] == "window":
        got = wr.kernel_public_lo(q, k, v, do, window=bound[1])
    else:
        ids = torch.ones(2, T, dtype=torch.long, device=DEV)
        ids[:, 99] = 0                                    # ends document 1
        assert torch.equal(document_lo(ids, 0), lo)
        got = wr.kernel_public_lo(q, k, v, do, kv_lo=document_lo(ids, 0))
    for t in got:
        assert torch.isfinite(t.float()).all()
    # LSE comes from the direct route, padded as the wrapper pads
    direct = wr.kernel_direct_lo(q, k, v, do, lo)
    for i, j in ((0, 0), (1, 2), (2, 3), (3, 4)):
        assert wr.bits_equal(got[i], direct[j]), ar.NAMES[j]
    rep, bad = wr.check_case_lo(tuple(t.cpu() for t in direct), c["ref"],
                                c["base"], c["lse_tol"])
    print("ATTN_RATIO window-F", f"D{D}T{T}{bound[0]}", json.dumps(ar.ratios(rep)),
          "lse", json.dumps(rep.get("lse")))
    assert not bad, bad


# ---------------------------------------------------------------------------
# G. GQA and MQA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
@pytest.mark.parametrize("D", DS)
def test_gqa(D, H, Hkv):
    c = wr.case("randn", 1, H, Hkv, 192, D, ("window", 33), seed=8)
    _check("G", f"D{D}H{H}kv{Hkv}", c, gqa=True)


# ---------------------------------------------------------------------------
# H. run to run
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_run_to_run_bitwise(D):
    c = wr.case("randn", *wr.BH, wr.BH[1], 256, D, "docs_T256")
    args = _dev(c)
    a = wr.kernel_direct_lo(*args)
    b = wr.kernel_direct_lo(*args)
    for name, x, y in zip(ar.NAMES, a, b):
        assert wr.bits_equal(x, y), name


# ---------------------------------------------------------------------------
# I. refusals and switches
# ---------------------------------------------------------------------------
def test_refusals():
    from saturn_amd.ops.flash import flash_attention

    ext = _ext()
    B, H, T, D = 2, 2, 128, 64
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=9)
    lo = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    o, lse = ext.attn_fwd(q, k, v, True, T, kv_lo=lo)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        flash_attention(q, k, v, causal=False, window=16)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, causal=False, kv_lo=lo)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, kv_lo=lo.long())
    bad = {
        "int32": lo.long(),
        "shape": lo[:, :-1].contiguous(),
        "shape ": torch.zeros(B + 1, T, dtype=torch.int32, device=DEV),
        "shape  ": torch.zeros(B, 1, T, dtype=torch.int32, device=DEV),
        "device": lo.cpu(),
        "contiguous": torch.zeros(B, 2 * T, dtype=torch.int32, device=DEV)[:, ::2],
    }
    for word, t in bad.items():
        with pytest.raises(RuntimeError, match=word.strip()):
            ext.attn_fwd(q, k, v, True, T, kv_lo=t)
        with pytest.raises(RuntimeError, match=word.strip()):
            ext.attn_bwd(do, q, k, v, o, lse, True, T, kv_lo=t)
    with pytest.raises(RuntimeError, match="causal"):
        ext.attn_fwd(q, k, v, False, T, kv_lo=lo)
    with pytest.raises(RuntimeError, match="causal"):
        ext.attn_bwd(do, q, k, v, o, lse, False, T, kv_lo=lo)
    # a [T] bound is the [B, T] bound with batch stride 0
    lo1 = wr.window_bound(T, 9).to(DEV)
    a = wr.kernel_direct_lo(q, k, v, do, lo1)
    b = wr.kernel_direct_lo(q, k, v, do, lo1.expand(B, T).contiguous())
    for name, x, y in zip(ar.NAMES, a, b):
        assert wr.bits_equal(x, y), name


# child time limit, by the rule of the switch children of
# test_attention_gpu.py: START_UP_S + FACTOR x the same work measured in
# this process (interpreter + torch import + device start-up and code-object
# load on a shared machine, then the work with 10x headroom)
START_UP_S = 120.0
FACTOR = 10.0
SWITCHES = ("SAMD_ATTN_V2", "SAMD_ATTN_BWD_TR16", "SAMD_ATTN_BWD_VL2",
            "SAMD_ATTN_DQ_GKV")
_state = {"seconds": None, "child_died": False}


def _own_seconds():
    if _state["seconds"] is None:
        wr.child_matrix(DEV)                          # warm
        res = wr.child_matrix(DEV)
        assert not res["failures"], res["failures"]
        assert res["path"] == _lo_paths(256, 128)
        _state["seconds"] = res["seconds"]
    return _state["seconds"]


def _child(mode, setting):
    if _state["child_died"]:
        pytest.skip("an earlier child ended by signal, abort or timeout: no "
                    "further child is started")
    if ar.device_error:
        pytest.fail("not started: device error earlier in this process: "
                    + ar.device_error[0])
    limit = START_UP_S + FACTOR * _own_seconds()
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    cmd = [sys.executable, os.path.abspath(wr.__file__), "--child", mode]
    try:
        p = subprocess.run(cmd, env=env, timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        _state["child_died"] = True
        pytest.fail(f"{setting}: child exceeded its {limit:.0f} s limit")
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if (p.returncode != 0 or not lines or "HIP error" in p.stderr
            or "hipError" in p.stderr):
        _state["child_died"] = True
        pytest.fail(f"{setting}: child status {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(lines[-1])


def test_child_vl2_is_refused_by_name():
    res = _child("refuse", {"SAMD_ATTN_BWD_VL2": "1"})
    assert res["refused"], res
    assert "SAMD_ATTN_BWD_VL2" in res["message"], res


def test_child_v2_off_takes_v1():
    res = _child("matrix", {"SAMD_ATTN_V2": "0"})
    print("ATTN_WINDOW_CHILD SAMD_ATTN_V2=0", json.dumps(res))
    assert res["path"].startswith("attn_fwd_kernel<128,1>"), res["path"]
    assert not res["failures"], res["failures"]


# ---------------------------------------------------------------------------
# J. model level, bitwise
# ---------------------------------------------------------------------------
def _llama(sliding_window):
    from saturn_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, n_ctx=192, n_embd=256, n_head=4,
                      n_kv_head=2, n_layer=2, ffn_dim=512,
                      sliding_window=sliding_window)
    return LlamaForCausalLM(cfg).to(device=DEV, dtype=torch.bfloat16)


def test_model_window_locality_bitwise():
    T, W = 192, 20
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(0))
    x = perm[:T].view(1, T).to(DEV)
    x2 = x.clone()
    x2[0, 0] = perm[T + 8].item()
    m = _llama(W)
    with torch.no_grad():
        a, b = m(x), m(x2)
    torch.cuda.synchronize()
    # every op but attention is row-wise; two layers of W-1 keys of reach
    far = 2 * (W - 1) + 1
    assert wr.bits_equal(a[:, far:], b[:, far:])
    assert not wr.bits_equal(a[:, :far], b[:, :far])
    with torch.no_grad():
        assert not wr.bits_equal(_llama(None)(x)[:, far:], a[:, far:])


def test_model_window_covering_T_is_the_plain_model():
    from saturn_amd.models.llama import llama_loss

    T = 192
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(1))
    x = perm[:T].view(1, T).to(DEV)       # distinct tokens: one add per row
    res = []
    for W in (None, T):
        m = _llama(W)
        logits = m(x)
        llama_loss(logits, x).backward()
        torch.cuda.synchronize()
        res.append((logits.detach(), {n: p.grad for n, p in m.named_parameters()}))
    assert wr.bits_equal(res[0][0], res[1][0])
    for n, g in res[0][1].items():
        assert g is not None and wr.bits_equal(g, res[1][1][n]), n
