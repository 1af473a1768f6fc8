"""Attention dropout fused into the K2 kernels (attention.hip's DROP
instantiations) on the GPU: the mask read out exactly from the forward and
from the dK/dV kernel, numerics against the fp64 reference of
tests/attn_dropout_ref.py under attn_ref's `close` criterion, and the bitwise
properties a counter-based mask must have.

Every shape has B*H <= 8 and T <= 512.  Each comparison prints an
``ATTN_RATIO dropout-<group> <case> <json>`` line (kernel error over the
error floor, per tensor); docs/kernels.md tabulates the worst per group.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import attn_dropout_ref as dr  # noqa: E402

from saturn_amd.ops import flash  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = dr.SEED


def _ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def _drop_paths(T, D):
    """What attn_dispatch(has_drop=True) must report with no switch set."""
    fwd = "attn_fwd_v2_kernel" if (T % 128 == 0 and D <= 128) else "attn_fwd_kernel"
    tr = 1 if D <= 128 else 0
    return (f"{fwd}<{D},0,1> attn_delta_kernel<{D}> "
            f"attn_bwd_kernel<{D},{tr},0,0,1> attn_dq_kernel<{D},{tr},0,0,1>")


def _check(group, name, c, gqa=False):
    """Both routes for a case; they must agree bit for bit (dk/dv under GQA
    excepted: fp32 atomics in arrival order); the public four and the direct
    LSE are checked."""
    direct, public = dr.run_case(c, DEV)
    assert dr.bits_equal(public[0], direct[0]), "out: routes differ"
    assert dr.bits_equal(public[1], direct[2]), "dq: routes differ"
    if not gqa:
        assert dr.bits_equal(public[2], direct[3]), "dk: routes differ"
        assert dr.bits_equal(public[3], direct[4]), "dv: routes differ"
    got = (public[0], direct[1]) + public[1:]
    rep, bad = dr.check_case_drop(got, c)
    print("ATTN_RATIO", f"dropout-{group}", name, json.dumps(ar.ratios(rep)),
          "lse", json.dumps(rep.get("lse")))
    assert not bad, bad
    return got


# ---------------------------------------------------------------------------
# A / B. the mask, read out exactly
# ---------------------------------------------------------------------------
# (T, D, forward variant reached)
READOUT = [(64, 64, "attn_fwd_kernel"), (192, 64, "attn_fwd_kernel"),
           (128, 64, "attn_fwd_v2_kernel"), (256, 128, "attn_fwd_v2_kernel"),
           (256, 256, "attn_fwd_kernel"), (512, 256, "attn_fwd_kernel")]
RB, RH = 2, 3


def _basis(T, D):
    """[T, D]: row j is 2^(j div D) e_(j mod D) (T/D <= 8: sums stay < 256)."""
    j = torch.arange(T)
    x = torch.zeros(T, D)
    x[j, j % D] = 2.0 ** (j // D)
    return x.bfloat16().expand(RB, RH, T, D).contiguous()


def _packed(keep, T, D, over_rows):
    """The integer the readout must give: sum over the keys j = d (mod D) of
    keep[.., i, j] 2^(j div D) as [B,H,T(i),D]; over_rows: the same over the
    rows i = d (mod D) as [B,H,T(j),D]."""
    w = _basis(T, D).float()                       # [B,H,T,D]
    k = keep.float()
    return torch.matmul(k.transpose(-1, -2) if over_rows else k, w)


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("T,D,variant", READOUT,
                         ids=[f"T{t}-D{d}" for t, d, _ in READOUT])
def test_forward_mask_readout(T, D, variant, causal, p):
    """q = 0 makes every seen probability 1/l exactly, so out * l / r is the
    integer whose bits are the keep flags: the forward's mask, bit for bit."""
    path = _ext().attn_dispatch(T, D, has_drop=True)
    assert path == _drop_paths(T, D)
    assert path.startswith(f"{variant}<{D},0,1>")
    assert ",1>" not in _ext().attn_dispatch(T, D).split()[0]
    q = torch.zeros(RB, RH, T, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(RB, RH, T, D, generator=torch.Generator().manual_seed(T + D)
                    ).bfloat16().to(DEV)
    v = _basis(T, D).to(DEV)
    o, lse = ar.launch_guard(_ext().attn_fwd)(q, k, v, causal, T,
                                              dropout_p=p, seed=SEED)
    keep, r = dr.keep_r(SEED, RB, RH, T, p)
    i = torch.arange(T)
    if causal:
        keep = keep & (i[None, :] <= i[:, None])
    l = (i + 1.0 if causal else torch.full((T,), float(T))).view(1, 1, T, 1)
    got = torch.round(o.float().cpu() * l / r)
    want = _packed(keep, T, D, over_rows=False)
    assert torch.equal(got, want), (got != want).nonzero()[:4]
    # LSE is the undropped one, log(l): an l that had lost a tenth of its
    # keys would be off by 0.1, fp32 exp/log by about 1e-6
    assert (lse.cpu() - torch.log(l.squeeze(-1))).abs().max() < 1e-3


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("T,D,variant", READOUT,
                         ids=[f"T{t}-D{d}" for t, d, _ in READOUT])
def test_dkdv_mask_readout(T, D, variant, p):
    """The same from the dK/dV kernel: with q = 0, full attention and
    dO[i] = 2^(i div D) e_(i mod D), dV[j] / (r bf16(1/T)) is the integer
    whose bits are the keep flags of column j — the transposed mask, so
    backward and forward agree on Z."""
    q = torch.zeros(RB, RH, T, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(RB, RH, T, D, generator=torch.Generator().manual_seed(T + D)
                    ).bfloat16().to(DEV)
    v = _basis(T, D).to(DEV)
    do = _basis(T, D).to(DEV)

    @ar.launch_guard
    def run():
        o, lse = _ext().attn_fwd(q, k, v, False, T, dropout_p=p, seed=SEED)
        return _ext().attn_bwd(do, q, k, v, o, lse, False, T, dropout_p=p,
                               seed=SEED)

    dq, dk, dv = run()
    keep, r = dr.keep_r(SEED, RB, RH, T, p)
    pb = torch.tensor(1.0 / T).bfloat16().float().item()   # the kernel's bf16 P
    got = torch.round(dv.float().cpu() / (r * pb))
    want = _packed(keep, T, D, over_rows=True)
    assert torch.equal(got, want), (got != want).nonzero()[:4]
    assert torch.isfinite(dq.float()).all() and torch.isfinite(dk.float()).all()


# ---------------------------------------------------------------------------
# C. numerics: D x T x mask x input kind x p
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "D,T,causal,kind,p", dr.MATRIX,
    ids=[f"D{d}-T{t}-{'c' if c else 'n'}-{k}-p{p}" for d, t, c, k, p in dr.MATRIX])
def test_matrix(D, T, causal, kind, p):
    assert _ext().attn_dispatch(T, D, has_drop=True) == _drop_paths(T, D)
    c = dr.case(kind, *dr.BH, dr.BH[1], T, D, causal, p)
    _check("C", f"D{D}-T{T}-{'c' if causal else 'n'}-{kind}-p{p}", c)


# ---------------------------------------------------------------------------
# D. ragged T through the public API
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [130, 197])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_ragged_T(D, T, causal):
    c = dr.case("randn", *dr.BH, dr.BH[1], T, D, causal, 0.1)
    got = _check("D", f"D{D}-T{T}-{'c' if causal else 'n'}", c)
    # the mask is the padded call's: the same rows through ext on inputs
    # padded by hand give the same bits
    q, k, v = (flash._pad_t64(c[n].to(DEV)) for n in ("q", "k", "v"))
    o, _ = ar.launch_guard(_ext().attn_fwd)(q, k, v, causal, T, dropout_p=0.1,
                                            seed=c["seed"])
    assert dr.bits_equal(o[:, :, :T].contiguous(), got[0].contiguous())


# ---------------------------------------------------------------------------
# E. GQA and MQA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_gqa(D, H, Hkv):
    c = dr.case("randn", 1, H, Hkv, 192, D, True, 0.1)
    _check("E", f"D{D}-H{H}kv{Hkv}", c, gqa=True)


# ---------------------------------------------------------------------------
# F. bitwise properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", dr.DS)
def test_run_to_run_bitwise(D):
    c = dr.case("randn", *dr.BH, dr.BH[1], 256, D, True, 0.1)
    a, _ = dr.run_case(c, DEV)
    b, _ = dr.run_case(c, DEV)
    for name, x, y in zip(ar.NAMES, a, b):
        assert dr.bits_equal(x, y), name
    # another seed is another mask
    q, k, v, do = (c[n].to(DEV) for n in ("q", "k", "v", "do"))
    other = dr.kernel_direct_drop(q, k, v, True, do, 0.1, c["seed"] + 1)
    assert not dr.bits_equal(other[0], a[0])
    assert dr.bits_equal(other[1], a[1])          # LSE does not see the mask


@pytest.mark.parametrize("T", [192, 256])
@pytest.mark.parametrize("D", dr.DS)
def test_p0_is_the_plain_call(D, T):
    q, k, v, do = ar.make_inputs("randn", 1, 2, 2, T, D, DEV, seed=4)
    plain = ar.kernel_public(q, k, v, True, do)

    @ar.launch_guard
    def run():
        ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = flash.flash_attention(ql, kl, vl, causal=True, dropout_p=0.0,
                                    seed=12345)
        out.backward(do)
        return out.detach(), ql.grad, kl.grad, vl.grad

    for x, y in zip(plain, run()):
        assert dr.bits_equal(x, y)
    # thr == 0 through ext launches the plain instantiations too
    o, lse = ar.launch_guard(_ext().attn_fwd)(q, k, v, True, T,
                                              dropout_p=2.0 ** -18, seed=7)
    assert dr.bits_equal(o.contiguous(), plain[0].contiguous())


@pytest.mark.parametrize("D", [64, 128])
def test_head_isolation_bitwise(D):
    """Replacing one head's inputs leaves every other (b, h) bit for bit."""
    B, H, T = 2, 3, 128
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=5)
    a = dr.kernel_direct_drop(q, k, v, True, do, 0.5, SEED)
    q2, k2, v2, do2 = (t.clone() for t in (q, k, v, do))
    for t in (q2, k2, v2, do2):
        t[1, 1] = torch.randn(T, D, device=DEV).bfloat16()
    b = dr.kernel_direct_drop(q2, k2, v2, True, do2, 0.5, SEED)
    for name, x, y in zip(ar.NAMES, a, b):
        for bb in range(B):
            for hh in range(H):
                same = dr.bits_equal(x[bb, hh], y[bb, hh])
                assert same == ((bb, hh) != (1, 1)), (name, bb, hh)


def test_all_dropped_rows_and_never_kept_keys():
    """p = 0.9, causal, T = 64: a row whose keys are all dropped gives
    out = 0 exactly (and, delta being 0, dS = 0: its dq row is 0 exactly);
    a key no row keeps gets dv = 0 exactly; everything is finite.

    dk of a never-kept key is NOT zero: the key still sits in the softmax
    denominator, dS = -P delta scale there, and the comparison with
    ref64_drop below covers it."""
    B, H, T, D, p = 2, 3, 64, 64, 0.9
    c = dr.case("randn", B, H, H, T, D, True, p)
    out, lse, dq, dk, dv = _check("F", "p0.9-T64", c)
    i = torch.arange(T)
    seen = c["keep"] & (i[None, :] <= i[:, None])
    dead_rows = ~seen.any(dim=-1)                  # [B,H,T]
    dead_keys = ~seen.any(dim=-2)
    assert dead_rows.sum() >= B * H and dead_keys.sum() >= B * H
    assert (out.cpu()[dead_rows] == 0).all()
    assert (dq.cpu()[dead_rows] == 0).all()
    assert (dv.cpu()[dead_keys] == 0).all()
    assert (dk.cpu()[dead_keys] != 0).any()
    for t in (out, lse, dq, dk, dv):
        assert torch.isfinite(t.float()).all()


# ---------------------------------------------------------------------------
# G. refusals, and the switches in a child process
# ---------------------------------------------------------------------------
def test_refusals():
    q, k, v, do = ar.make_inputs("randn", 1, 2, 2, 64, 64, DEV, seed=1)
    ext = _ext()
    lo = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="dropout_p"):
        ext.attn_fwd(q, k, v, True, 64, dropout_p=1.0, seed=1)
    with pytest.raises(RuntimeError, match="dropout_p"):
        ext.attn_fwd(q, k, v, True, 64, dropout_p=-0.5, seed=1)
    with pytest.raises(RuntimeError, match="kv_lo"):
        ext.attn_fwd(q, k, v, True, 64, kv_lo=lo, dropout_p=0.1, seed=1)
    o, lse = ext.attn_fwd(q, k, v, True, 64)
    with pytest.raises(RuntimeError, match="kv_lo"):
        ext.attn_bwd(do, q, k, v, o, lse, True, 64, kv_lo=lo, dropout_p=0.1,
                     seed=1)
    with pytest.raises(RuntimeError, match="kv_lo"):
        ext.attn_dispatch(64, 64, has_lo=True, has_drop=True)
    for kw in (dict(window=8), dict(kv_lo=lo)):
        with pytest.raises(ValueError):
            flash.flash_attention(q, k, v, causal=True, dropout_p=0.1, **kw)
    with pytest.raises(ValueError):
        flash.flash_attention(q, k, v, causal=True, dropout_p=1.0)
    torch.cuda.synchronize()


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
        dr.child_matrix(DEV)                          # warm
        res = dr.child_matrix(DEV)
        assert not res["failures"], res["failures"]
        assert res["path"] == _drop_paths(256, 128)
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
    cmd = [sys.executable, os.path.abspath(dr.__file__), "--child", mode]
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
    print("ATTN_DROPOUT_CHILD SAMD_ATTN_V2=0", json.dumps(res))
    assert res["path"].startswith("attn_fwd_kernel<128,0,1>"), res["path"]
    assert not res["failures"], res["failures"]


# ---------------------------------------------------------------------------
# H. model level
# ---------------------------------------------------------------------------
def _gptj(**kw):
    from saturn_amd.models.gptj import GPTJConfig, GPTJForCausalLM

    torch.manual_seed(0)
    cfg = GPTJConfig(vocab_size=512, n_ctx=128, n_embd=256, n_head=4,
                     n_layer=2, rotary_dim=32, **kw)
    return GPTJForCausalLM(cfg).to(device=DEV, dtype=torch.bfloat16)


def test_model_trains_with_attn_pdrop():
    from saturn_amd.models.gptj import pretraining_loss
    from saturn_amd.ops.optim import FusedSGD

    x = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(2)
                      ).to(DEV)
    model = _gptj(attn_pdrop=0.1).train()
    h = torch.zeros(2, 128, 256, device=DEV, dtype=torch.bfloat16)
    plain = _gptj().train()
    # the plain model takes the block node here (unless switched off); with
    # dropout the block leaves it in training and returns to it in eval
    off = "0" in (os.environ.get("SAMD_MLP_FUSED"), os.environ.get("SAMD_BLOCK_FUSED"))
    assert plain.h[0]._use_fused(h) is (not off)
    assert model.h[0]._use_fused(h) is False
    assert model.eval().h[0]._use_fused(h) is (not off)
    model.train()
    opt = FusedSGD(model.parameters(), lr=1e-3)
    loss = pretraining_loss(model(x), x)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    lv = loss.item()
    assert lv == lv and lv < 20.0, lv
    assert all(torch.isfinite(p.grad.float()).all() for p in model.parameters()
               if p.grad is not None)
    # two training forwards differ; eval equals the attn_pdrop = 0 model
    model2 = _gptj(attn_pdrop=0.1).train()
    assert not torch.equal(model2(x), model2(x))
    assert torch.equal(model2.eval()(x), plain.eval()(x))


def test_model_attn_pdrop_zero_is_the_present_path():
    x = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(2)
                      ).to(DEV)
    zero, plain = _gptj(attn_pdrop=0.0).train(), _gptj().train()
    h = torch.zeros(2, 128, 256, device=DEV, dtype=torch.bfloat16)
    off = "0" in (os.environ.get("SAMD_MLP_FUSED"), os.environ.get("SAMD_BLOCK_FUSED"))
    assert zero.h[0]._use_fused(h) is (not off)
    assert plain.h[0]._use_fused(h) is (not off)
    assert torch.equal(zero(x), plain(x))
