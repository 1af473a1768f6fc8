"""The stored-dS dQ route of attn_bwd at D = 256 (attention.hip:
attn_bwd_kernel<256,0,0,0,0,1> + attn_dq_ds_kernel<256>).

The route must give the bits of the recompute route (attn_dq_kernel), so
every comparison here is torch.equal on dq, dk and dv between dq_route=1 and
dq_route=0 on the same inputs: no tolerance.  The recompute route itself is
held to the fp64 reference by tests/test_attention_gpu.py.

    python tests/test_attention_dq_ds_gpu.py --child     # one JSON line

is the child of test_switch_off_in_child_process.
"""

import json
import os
import subprocess
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402  (plain helper modules beside this file)
import attn_run as run  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256
SWITCH = "SAMD_ATTN_DQ_DS"
BOUND_BYTES = 128 << 20
DS_NAMES = ("attn_fwd_kernel<256> attn_delta_kernel<256> "
            "attn_bwd_kernel<256,0,0,0,0,1> attn_dq_ds_kernel<256>")
GRADS = ("dq", "dk", "dv")


@run.launch_guard
def _fwd(q, k, v, causal, kv_len):
    return run.ext().attn_fwd(q, k, v, causal, kv_len)


@run.launch_guard
def _bwd(do, q, k, v, o, lse, causal, kv_len, **kw):
    return run.ext().attn_bwd(do, q, k, v, o, lse, causal, kv_len, **kw)


def _padded(kind, B, H, T, seed):
    """(q, k, v, do) of make_inputs at T, zero-padded to a multiple of 64 the
    way the public wrapper pads; T is then the kv_len of the call."""
    from saturn_amd.ops.flash import _pad_t64

    return tuple(_pad_t64(t) for t in ar.make_inputs(kind, B, H, H, T, D, DEV,
                                                     seed=seed))


def _routes_equal(q, k, v, do, causal, kv_len, **kw1):
    """attn_bwd with dq_route=0 and with dq_route=1 (+ kw1): the three
    gradients must be the same bits.  Returns the stored-dS route's."""
    o, lse = _fwd(q, k, v, causal, kv_len)
    want = _bwd(do, q, k, v, o, lse, causal, kv_len, dq_route=0)
    got = _bwd(do, q, k, v, o, lse, causal, kv_len, dq_route=1, **kw1)
    for n, a, b in zip(GRADS, got, want):
        assert a.shape == b.shape and a.stride() == b.stride(), n
        assert torch.equal(a, b), f"{n}: stored-dS route differs from recompute"
        assert run.bits_equal(a, b), f"{n}: differs in the sign of a zero"
    return got


# ---------------------------------------------------------------------------
# bitwise equality of the routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["randn", "peaky"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [64, 128, 192, 320])   # one key block, the block
#                                                      edge, odd tile counts
@pytest.mark.parametrize("B,H", [(1, 3), (2, 2)])
def test_routes_bitwise(B, H, T, causal, kind):
    q, k, v, do = ar.make_inputs(kind, B, H, H, T, D, DEV, seed=21)
    _routes_equal(q, k, v, do, causal, T)


@pytest.mark.parametrize("causal", [True, False])
def test_routes_bitwise_strided(causal):
    """q/k/v/dout as the model passes them: [B, T, H, D] storage seen through
    transpose(1, 2)."""
    B, H, T = 2, 2, 192
    q, k, v, do = (t.transpose(1, 2).contiguous().transpose(1, 2)
                   for t in ar.make_inputs("randn", B, H, H, T, D, DEV, seed=22))
    assert not q.is_contiguous() and q.stride(3) == 1
    _routes_equal(q, k, v, do, causal, T)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [130, 257])            # -> 192, 320
def test_routes_bitwise_kv_len(T, causal):
    q, k, v, do = _padded("randn", 2, 2, T, seed=23)
    assert q.shape[2] == ar.padded_t(T) > T
    _routes_equal(q, k, v, do, causal, T)


# ---------------------------------------------------------------------------
# poisoned scratch: every dS element the dQ kernel reads was written by the
# dK/dV kernel of the same call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [192, 130, 257])       # kv_len == T and < T
def test_poisoned_scratch(T, causal):
    B, H = 2, 2
    q, k, v, do = _padded("randn", B, H, T, seed=24)
    Tp = q.shape[2]
    scratch = torch.full((B * H * Tp * Tp,), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
    assert bool(scratch.isnan().all())
    dq, _, _ = _routes_equal(q, k, v, do, causal, T, ds_scratch=scratch)
    assert bool(torch.isfinite(dq).all())
    # the scratch was used: the call wrote into it
    assert not bool(scratch.isnan().all())


# ---------------------------------------------------------------------------
# auto route and the size bound
# ---------------------------------------------------------------------------
def test_auto_route_small_takes_stored_ds():
    for n in run.SWITCHES + (SWITCH,):
        assert n not in os.environ, f"{n} is set: this test is about the default"
    B, H, T = 2, 2, 128
    assert run.ext().attn_ds_eligible(B, H, H, T, D)
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=25)
    o, lse = _fwd(q, k, v, True, T)
    # a poisoned scratch tells the routes apart even though their bits agree:
    # the auto route must have written into it
    scratch = torch.full((B * H * T * T,), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
    auto = _bwd(do, q, k, v, o, lse, True, T, ds_scratch=scratch)
    assert not bool(scratch.isnan().all())
    one = _bwd(do, q, k, v, o, lse, True, T, dq_route=1)
    for n, a, b in zip(GRADS, auto, one):
        assert torch.equal(a, b), n


def test_bound_rule():
    """B*H*T*T*2 <= 128 MiB.  B*H = 16 at T = 2048 is exactly 128 MiB, the
    largest eligible call; one more head exceeds it."""
    el = run.ext().attn_ds_eligible
    assert 16 * 2048 * 2048 * 2 == BOUND_BYTES
    assert el(16, 16, 16, 512, D)                    # the flagship: 128 MiB
    assert el(1, 16, 16, 2048, D) and el(16, 1, 1, 2048, D)
    assert not el(1, 17, 17, 2048, D)
    assert not el(16, 16, 16, 576, D)
    assert not el(32, 16, 16, 512, D)
    assert el(2, 2, 2, 128, D)
    assert not el(2, 2, 2, 128, 128) and not el(2, 2, 2, 128, 64)
    assert not el(2, 4, 2, 128, D)                   # GQA
    assert not el(2, 2, 2, 128, D, has_lo=True)
    assert not el(2, 2, 2, 128, D, has_drop=True)


def test_oversized_call_keeps_recompute():
    """Backward only, B*H = 17 at T = 2048 (136 MiB of dS): the auto route is
    the recompute route bit for bit, and dq_route=1 is refused by name.  (At
    B*H = 16 the scratch is exactly the bound and the call is eligible.)"""
    B, H, T = 1, 17, 2048
    assert B * H * T * T * 2 > BOUND_BYTES
    g = torch.Generator(device=DEV).manual_seed(26)
    q, k, v, do = (torch.randn(B, H, T, D, device=DEV, generator=g)
                   .to(torch.bfloat16) for _ in range(4))
    o, lse = _fwd(q, k, v, True, T)
    scratch = torch.full((B * H * T * T,), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
    auto = _bwd(do, q, k, v, o, lse, True, T, ds_scratch=scratch)
    assert bool(scratch.isnan().all())               # the recompute route ran
    zero = _bwd(do, q, k, v, o, lse, True, T, dq_route=0)
    for n, a, b in zip(GRADS, auto, zero):
        assert torch.equal(a, b), n
    with pytest.raises(RuntimeError) as e:
        run.ext().attn_bwd(do, q, k, v, o, lse, True, T, dq_route=1)
    msg = str(e.value).splitlines()[0]
    assert msg.startswith("attn_bwd:") and "128 MiB" in msg, msg
    torch.cuda.synchronize()


def test_call_at_the_bound_is_eligible():
    """B*H = 16, T = 2048: exactly 128 MiB, taken by the stored-dS route."""
    B, H, T = 1, 16, 2048
    g = torch.Generator(device=DEV).manual_seed(27)
    q, k, v, do = (torch.randn(B, H, T, D, device=DEV, generator=g)
                   .to(torch.bfloat16) for _ in range(4))
    _routes_equal(q, k, v, do, True, T)


# ---------------------------------------------------------------------------
# refusals, on the host and before any launch
# ---------------------------------------------------------------------------
def _small(H=2, Hkv=None, d=D, T=128, seed=28):
    q, k, v, do = ar.make_inputs("randn", 1, H, Hkv or H, T, d, DEV, seed=seed)
    o, lse = _fwd(q, k, v, True, T)
    return (do, q, k, v, o, lse, True, T)


def _refused(args, word, **kw):
    with pytest.raises(RuntimeError) as e:
        run.ext().attn_bwd(*args, **kw)
    msg = str(e.value).splitlines()[0]
    assert msg.startswith("attn_bwd:") and word in msg, msg
    torch.cuda.synchronize()                         # and nothing was launched


def test_refuses_kv_lo():
    lo = ar.window_bound(128, 32).to(DEV)
    _refused(_small(), "kv_lo", kv_lo=lo, dq_route=1)


def test_refuses_dropout():
    _refused(_small(), "dropout_p", dropout_p=0.1, seed=1, dq_route=1)


def test_refuses_gqa():
    _refused(_small(H=4, Hkv=2), "Hkv", dq_route=1)


def test_refuses_d128():
    _refused(_small(d=128), "D == 256", dq_route=1)


def test_refuses_bad_route_value():
    _refused(_small(), "dq_route", dq_route=2)


BAD_SCRATCH = [
    ("small", lambda n: torch.empty(n - 1, device=DEV, dtype=torch.bfloat16)),
    ("fp16", lambda n: torch.empty(n, device=DEV, dtype=torch.float16)),
    ("cpu", lambda n: torch.empty(n, dtype=torch.bfloat16)),
    ("strided", lambda n: torch.empty(2 * n, device=DEV,
                                      dtype=torch.bfloat16)[::2]),
]


@pytest.mark.parametrize("what,make", BAD_SCRATCH,
                         ids=[w for w, _ in BAD_SCRATCH])
def test_refuses_bad_scratch(what, make):
    args = _small()
    _refused(args, "ds_scratch", dq_route=1, ds_scratch=make(1 * 2 * 128 * 128))


# ---------------------------------------------------------------------------
# names and the switch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 192, 512])
def test_dispatch_names(T):
    ext = run.ext()
    assert ext.attn_dispatch(T, D) == (
        "attn_fwd_kernel<256> attn_delta_kernel<256> "
        "attn_bwd_kernel<256,0,0> attn_dq_kernel<256,0,0>")
    assert ext.attn_dispatch(T, D, ds_route=True) == DS_NAMES
    assert ext.attn_dispatch(T, D, has_lo=False, has_drop=False,
                             ds_route=True) == DS_NAMES


@pytest.mark.parametrize("kw,word", [
    (dict(T=128, D=128), "D == 256"), (dict(T=128, D=64), "D == 256"),
    (dict(T=128, D=256, has_lo=True), "kv_lo"),
    (dict(T=128, D=256, has_drop=True), "dropout_p"),
    (dict(T=16384, D=256), "128 MiB"),               # 512 MiB for one head
], ids=["D128", "D64", "kv_lo", "dropout", "T16384"])
def test_dispatch_refuses(kw, word):
    with pytest.raises(RuntimeError) as e:
        run.ext().attn_dispatch(ds_route=True, **kw)
    assert word in str(e.value).splitlines()[0]


def child_work():
    """Auto route, dq_route=0 and dq_route=1 at (2, 2, 128); with a poisoned
    scratch handed to the auto call, so that the route it took is visible."""
    t0 = time.perf_counter()
    B, H, T = 2, 2, 128
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=25)
    o, lse = _fwd(q, k, v, True, T)
    scratch = torch.full((B * H * T * T,), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
    auto = _bwd(do, q, k, v, o, lse, True, T, ds_scratch=scratch)
    zero = _bwd(do, q, k, v, o, lse, True, T, dq_route=0)
    one = _bwd(do, q, k, v, o, lse, True, T, dq_route=1)
    return {"auto_equals_route0": all(torch.equal(a, b)
                                      for a, b in zip(auto, zero)),
            "route1_equals_route0": all(torch.equal(a, b)
                                        for a, b in zip(one, zero)),
            "auto_wrote_scratch": not bool(scratch.isnan().all()),
            "names": run.ext().attn_dispatch(T, D),
            "seconds": round(time.perf_counter() - t0, 3)}


def test_switch_off_in_child_process():
    """SAMD_ATTN_DQ_DS=0 (read once per process): the auto route is the
    recompute route; dq_route=1 still asks for the stored-dS kernels."""
    if run.child_died:
        pytest.skip("no further child is started: " + run.child_died[0])
    if run.device_error:
        pytest.fail("not started: device error earlier in this process: "
                    + run.device_error[0])
    child_work()
    own = child_work()                               # second run: code loaded
    assert own["auto_wrote_scratch"] and own["auto_equals_route0"]
    limit = run.START_UP_S + run.LIMIT_FACTOR * own["seconds"]
    env = {k: v for k, v in os.environ.items()
           if k not in run.SWITCHES + (SWITCH,)}
    env[SWITCH] = "0"
    cmd = [sys.executable, os.path.abspath(__file__), "--child"]
    try:
        p = subprocess.run(cmd, env=env, timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        run.child_died.append(f"{SWITCH}=0 child exceeded its {limit:.0f} s limit")
        pytest.fail(run.child_died[-1])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if (p.returncode != 0 or not lines or "HIP error" in p.stderr
            or "hipError" in p.stderr):
        run.child_died.append(f"{SWITCH}=0 child ended with status {p.returncode}")
        pytest.fail(f"child status {p.returncode}, {len(lines)} result "
                    f"line(s)\n{p.stderr[-2000:]}")
    res = json.loads(lines[-1])
    print("ATTN_DQ_DS child", json.dumps(res))
    assert res["auto_equals_route0"]
    assert not res["auto_wrote_scratch"]             # the recompute route ran
    assert res["route1_equals_route0"]
    assert res["names"] == own["names"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--child"]:
        sys.exit("usage: test_attention_dq_ds_gpu.py --child")
    print(json.dumps(child_work()), flush=True)
