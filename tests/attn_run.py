"""Everything of the attention tests that touches the device: the guarded
routes into the kernels (ext.attn_fwd / ext.attn_bwd directly, and the public
flash_attention), the bitwise comparison, and the child processes that run a
fixed piece of work under one setting of the environment switches (they are
read once per process, so each setting needs a process of its own):

    python tests/attn_run.py --child sweep|window-matrix|window-refuse|
                                     drop-matrix|drop-refuse

Each child prints one JSON line.  Reference, floor and criterion are
tests/attn_ref.py's.  This is a plain module: no tests, no fixtures.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402


def ext():
    from saturn_amd.ops import require_ext

    return require_ext()


# ---------------------------------------------------------------------------
# running the kernels
# ---------------------------------------------------------------------------
device_error = []


def launch_guard(fn):
    """After a device error (they are sticky and surface at the next
    synchronise) nothing more is launched from this process: every later
    call fails at once instead of queueing work on a faulted device."""
    def wrapped(*args, **kw):
        if device_error:
            raise RuntimeError("not launched: earlier device error: "
                               + device_error[0])
        try:
            res = fn(*args, **kw)
            torch.cuda.synchronize()
            return res
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                device_error.append(str(e).splitlines()[0])
            raise
    wrapped.__doc__ = fn.__doc__
    return wrapped


def _set(p=0.0, seed=0, **kw):
    """The keywords that are set: a plain call stays the plain call."""
    kw = {n: x for n, x in kw.items() if x is not None}
    if p > 0.0:
        kw.update(dropout_p=p, seed=seed)
    return kw


@launch_guard
def kernel_direct(q, k, v, causal, do, *, lo=None, p=0.0, seed=0):
    """ext.attn_fwd / ext.attn_bwd on inputs padded the way the wrapper pads
    them (a bound with T - 1, the last real key); all five results sliced
    back to T.  The only route to LSE."""
    from saturn_amd.ops.flash import _pad_t64

    T = q.shape[2]
    qp, kp, vp, dop = (_pad_t64(t) for t in (q, k, v, do))
    if lo is not None:
        lo = torch.nn.functional.pad(lo, (0, (-T) % 64), value=T - 1).contiguous()
    kw = _set(p, seed, kv_lo=lo)
    o, lse = ext().attn_fwd(qp, kp, vp, causal, T, **kw)
    dq, dk, dv = ext().attn_bwd(dop, qp, kp, vp, o, lse, causal, T, **kw)
    return tuple(t[:, :, :T] for t in (o, lse, dq, dk, dv))


@launch_guard
def kernel_public(q, k, v, causal, do, *, window=None, lo=None, p=0.0, seed=0):
    """flash_attention + autograd on fresh leaves: (out, dq, dk, dv)."""
    from saturn_amd.ops.flash import flash_attention

    kw = _set(p, seed, window=window, kv_lo=lo)
    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = flash_attention(ql, kl, vl, causal=causal, **kw)
    out.backward(do)
    return out.detach(), ql.grad, kl.grad, vl.grad


@launch_guard
def flash_fwd_bwd(q, k, v, causal, do):
    """flash_attention + backward on the caller's own tensors (views of
    leaves, any layout); the gradients land in the caller's leaves."""
    from saturn_amd.ops.flash import flash_attention

    out = flash_attention(q, k, v, causal=causal)
    out.backward(do)
    return out.detach()


@launch_guard
def ext_fwd_bwd(q, k, v, causal, do, kv_len):
    """ext.attn_fwd / ext.attn_bwd as given (T a multiple of 64, explicit
    kv_len), nothing padded or sliced: (out, lse, dq, dk, dv)."""
    o, lse = ext().attn_fwd(q, k, v, causal, kv_len)
    dq, dk, dv = ext().attn_bwd(do, q, k, v, o, lse, causal, kv_len)
    return o, lse, dq, dk, dv


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
        b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def on_device(c, device="cuda"):
    """(q, k, v, causal, do) and the route keywords of an attn_ref.case."""
    q, k, v, do = (c[n].to(device) for n in ("q", "k", "v", "do"))
    lo = None if c["lo"] is None else c["lo"].to(device)
    return (q, k, v, c["causal"], do), {"lo": lo, "p": c["p"], "seed": c["seed"]}


def both_routes(c, gqa=False, device="cuda"):
    """Both routes for an attn_ref.case or a (q, k, v, causal, do) tuple:
    (direct five, public four).  The public wrapper gives out and the
    gradients (shape and leaf plumbing), the direct calls LSE; the two must
    agree bit for bit, except for dk/dv under GQA, which are summed with
    fp32 atomics in arrival order."""
    args, kw = on_device(c, device) if isinstance(c, dict) else (c, {})
    q, k, v = args[:3]
    public = kernel_public(*args, **kw)
    direct = kernel_direct(*args, **kw)
    for t, like in zip(public, (q, q, k, v)):
        assert t.shape == like.shape, (t.shape, like.shape)
    for i, j in ((0, 0), (1, 2), (2, 3), (3, 4)):
        if not (gqa and R.NAMES[j] in ("dk", "dv")):
            assert bits_equal(public[i], direct[j]), f"{R.NAMES[j]}: routes differ"
    return direct, public


# ---------------------------------------------------------------------------
# the work of the children
#   sweep          a compact subset of the plain path matrix, the ragged and
#                  the GQA groups, checked
#   window-matrix  the T=256, D=128 cases of the kv_lo matrix, both routes,
#   drop-matrix    and the same of the dropout matrix, checked
#   *-refuse       the matrix's first case must be refused by attn_bwd;
#                  reports the message
# ---------------------------------------------------------------------------
SWEEP_CASES = [
    # (B, H, Hkv, T, D): a v1-shape T, a v2-shape T and a ragged T per D ...
    *[(1, 3, 3, T, D) for D in (64, 128, 256) for T in (192, 256, 197)],
    # ... and one GQA case (ragged, so kv_len masking and atomics combine)
    (1, 6, 2, 197, 128),
]
WINDOW_CHILD_CASES = [(128, b, "randn") for b in ("W65_T256", "docs_T256")]
DROP_CHILD_CASES = [(128, 256, causal, "randn", 0.1) for causal in (True, False)]


def sweep(device="cuda"):
    t0 = time.perf_counter()
    cases, failures, paths, digest = {}, [], {}, 0
    for (B, H, Hkv, T, D) in SWEEP_CASES:
        paths[f"T{R.padded_t(T)}_D{D}"] = ext().attn_dispatch(R.padded_t(T), D)
        for causal in (True, False):
            name = f"B{B}H{H}kv{Hkv}T{T}D{D}{'c' if causal else 'n'}"
            q, k, v, do = R.make_inputs("randn", B, H, Hkv, T, D, device, seed=7)
            got = kernel_direct(q, k, v, causal, do)
            rep, bad = R.check_plain(got, q, k, v, causal, do)
            cases[name] = R.ratios(rep)
            failures += [f"{name}: {b}" for b in bad]
            if Hkv == H:        # bitwise reproducible outputs only
                for t in got:
                    bits = t.contiguous().view(
                        torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
                    digest = (digest * 31 + int(bits.long().sum())) % (1 << 61)
    torch.cuda.synchronize()
    # digest: informational, shows whether a setting changed any output bit
    return {"cases": cases, "paths": paths, "failures": failures,
            "digest": digest, "seconds": round(time.perf_counter() - t0, 3)}


def child_cases(what):
    """[(label, case)] of the window or the drop children."""
    if what == "window":
        return [(b, R.case(kind, *R.BH_WINDOW, R.BH_WINDOW[1], R.BOUNDS[b][0],
                           D, bound=b))
                for D, b, kind in WINDOW_CHILD_CASES]
    return [(f"causal={causal}",
             R.case(kind, *R.BH_DROP, R.BH_DROP[1], T, D, causal, p=p,
                    seed=R.DROP_INPUT_SEED))
            for D, T, causal, kind, p in DROP_CHILD_CASES]


def child_matrix(what, device="cuda"):
    t0 = time.perf_counter()
    failures = []
    for label, c in child_cases(what):
        try:
            direct, _ = both_routes(c, device=device)
        except AssertionError as e:
            failures.append(f"{label}: {e}")
            continue
        _, bad = R.check_case(direct, c["ref"], c["base"], c["lse_tol"])
        failures += [f"{label}: {b}" for b in bad]
    flag = {"has_lo": True} if what == "window" else {"has_drop": True}
    return {"failures": failures,
            "path": ext().attn_dispatch(256, 128, **flag),
            "seconds": round(time.perf_counter() - t0, 3)}


def child_refuse(what, device="cuda"):
    args, kw = on_device(child_cases(what)[0][1], device)
    try:
        kernel_direct(*args, **kw)
    except RuntimeError as e:
        return {"refused": True, "message": str(e).splitlines()[0]}
    return {"refused": False, "message": ""}


MODES = {
    "sweep": sweep,
    "window-matrix": lambda: child_matrix("window"),
    "window-refuse": lambda: child_refuse("window"),
    "drop-matrix": lambda: child_matrix("drop"),
    "drop-refuse": lambda: child_refuse("drop"),
}


def main(argv):
    if len(argv) != 2 or argv[0] != "--child" or argv[1] not in MODES:
        print("usage: attn_run.py --child " + "|".join(MODES), file=sys.stderr)
        return 2
    res = MODES[argv[1]]()
    print(json.dumps(res), flush=True)
    return 1 if argv[1] == "sweep" and res["failures"] else 0


# ---------------------------------------------------------------------------
# the parent's side
# ---------------------------------------------------------------------------
SWITCHES = ("SAMD_ATTN_V2", "SAMD_ATTN_BWD_TR16", "SAMD_ATTN_BWD_VL2",
            "SAMD_ATTN_DQ_GKV")
# child time limit = START_UP_S + LIMIT_FACTOR x the same work measured in
# the parent process: interpreter + torch import + device start-up and
# code-object load on a shared machine, then the work with 10x headroom
START_UP_S = 120.0
LIMIT_FACTOR = 10.0
child_died = []
_own = {}


def own_run(mode):
    """MODE's work in this process, the second of two runs (code objects
    loaded), once per process: its "seconds" size the children's limit."""
    if mode not in _own:
        MODES[mode]()
        res = MODES[mode]()
        assert not res["failures"], res["failures"]
        _own[mode] = res
    return _own[mode]


def run_child(mode, setting, own_seconds):
    """Run MODE in a fresh process under the switches of `setting`:
    (its JSON result, its exit status, the time limit).  A child that ends
    by signal, abort or timeout, exits non-zero where zero is required
    (every mode but sweep, whose status 1 reports failed cases), prints no
    result or reports a device error is the last one started from this
    pytest process, whichever test file asks for the next."""
    import pytest

    if child_died:
        pytest.skip("no further child is started: " + child_died[0])
    if device_error:
        pytest.fail("not started: device error earlier in this process: "
                    + device_error[0])
    limit = START_UP_S + LIMIT_FACTOR * own_seconds
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode]
    try:
        p = subprocess.run(cmd, env=env, timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        child_died.append(f"{mode} {setting} exceeded its {limit:.0f} s limit")
        pytest.fail(f"{setting}: child exceeded its {limit:.0f} s limit")
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if (p.returncode < 0 or p.returncode == 134
            or (mode != "sweep" and p.returncode != 0) or not lines
            or "HIP error" in p.stderr or "hipError" in p.stderr):
        # no result line: the work did not finish (a device error surfaces
        # as an exception, status 1): treated like a signal
        child_died.append(f"{mode} {setting} ended with status {p.returncode}")
        pytest.fail(f"{setting}: child status {p.returncode}, "
                    f"{len(lines)} result line(s)\n{p.stderr[-2000:]}")
    return json.loads(lines[-1]), p.returncode, limit


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
