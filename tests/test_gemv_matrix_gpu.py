"""GPU: every decode-GEMV path against the fp64 reference of
gemv_reference.py, under its derived bound (no tolerance is set here).

The matrix (gemv_reference.matrix_cases) walks launch_gemv's dispatch, the
row clamps, the grid-stride wrap above the 4096-block cap, the fused norms,
the epilogues, the three weight formats, the SwiGLU pair kernels and the MoE
expert indirection.  Every output is the [:M] view of a sentinel-filled
buffer: rows >= M must keep the sentinel and no row < M may.  Exact-decode
tests pin the fp8 lo/hi and the int4 nibble order by equality, the host
guards are shown to refuse before any launch, and one child process covers
the MDI_GEMV_PRE=1 kernel (the flag is read once per process).

Each case prints its worst err/bound; profiles/gemv_error_margins.md keeps
the per-family figures of one run.
"""

import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import gemv_reference as R
from gemv_reference import (EPS, SENTINEL, check_out_buffer, gemv_error_ok,
                            make_inputs, matrix_cases, reference, run_case)

pytestmark = pytest.mark.gpu

if os.environ.get("MDI_GEMV_GRID_CAP") or os.environ.get("MDI_GEMV_PRE"):
    pytest.skip("MDI_GEMV_GRID_CAP / MDI_GEMV_PRE change the dispatch this "
                "module assumes", allow_module_level=True)

DEV = "cuda:0"
CASES = {c.id: c for c in matrix_cases()}
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_gemv_matrix(ops, name):
    case = CASES[name]
    inp = make_inputs(case)
    ref = reference(case, inp)
    buf = run_case(ops, case, inp, DEV)
    torch.cuda.synchronize()
    ok, worst, msg = check_out_buffer(buf, case.M, ref, case.K)
    print(f"{name} [{case.dispatch().kernel}]: max err/bound = {worst:.3f}")
    assert ok, f"{name}: {msg}"


# ---------------------------------------------------------------------------
# exact decode (equality, no bound)
def test_fp8_decode_exact(ops):
    """Every finite e4m3fn code through the packed converts: one-hot x at
    each of the 16 positions of a lane's load picks out decode(code)."""
    codes = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F],
                         dtype=torch.uint8)
    assert codes.numel() == 254
    r = torch.arange(254)[:, None]
    p = torch.arange(16)[None, :]
    W = codes[(r + 17 * p) % 254].contiguous()   # differs along every row
    want = R.fp8_decode(W)
    assert torch.isfinite(want).all()
    Wd = W.to(DEV)
    ones = torch.ones(254, device=DEV)
    for pos in range(16):
        x = torch.zeros(16, dtype=BF, device=DEV)
        x[pos] = 1.0
        buf = R.new_out_buffer(254, DEV)
        ops.gemv_fp8(buf[:254], Wd, ones, x, None, None, 0)
        got = buf.float().cpu()
        assert torch.equal(got[:254], want[:, pos]), pos
        assert bool((got[254:] == SENTINEL).all())


def test_int4_decode_exact(ops):
    """Distinct nibble codes, scale 1, zero 0: one-hot x at each of the 32
    positions of a 16-byte load picks out the nibble itself."""
    M, K = 16, 32
    r = torch.arange(M)[:, None]
    k = torch.arange(K)[None, :]
    nib = torch.zeros(M, 128, dtype=torch.uint8)
    nib[:, :K] = ((r + 3 * k + k // 8) % 16).to(torch.uint8)
    packed = R.int4_pack(nib).to(DEV)
    qp = torch.tensor([1.0, 0.0], dtype=BF).repeat(M, 1, 1).to(DEV)
    for pos in range(K):
        x = torch.zeros(K, dtype=BF, device=DEV)
        x[pos] = 1.0
        buf = R.new_out_buffer(M, DEV)
        ops.gemv_int4(buf[:M], packed, qp, x, None, None, 0)
        got = buf.float().cpu()
        assert torch.equal(got[:M], nib[:, pos].float()), pos
        assert bool((got[M:] == SENTINEL).all())


# ---------------------------------------------------------------------------
# norms and the SwiGLU glue
def _padded(n, device=DEV):
    return torch.full((n + R.PAD_ROWS,), SENTINEL, dtype=BF, device=device)


def _check_flat(buf, n, r, K, label):
    got = buf.float().cpu()
    ok, ratio = gemv_error_ok(got[:n], r.ref.flatten(), r.A.flatten(), K)
    print(f"{label}: max err/bound = {float(ratio.max()):.3f}")
    assert bool((got[n:] == SENTINEL).all()), f"{label}: wrote past the end"
    assert ok, f"{label}: err/bound {float(ratio.max()):.3g}"


def _norm_inputs(n, batch):
    g = torch.Generator().manual_seed(1000 * n + batch)
    x = ((torch.randn(batch, n, generator=g) + 0.5) * 0.01).to(BF)
    w = (torch.randn(n, generator=g)
         * (0.25 + 1.5 * torch.rand(n, generator=g))).to(BF)
    b = torch.randn(n, generator=g).to(BF)
    return x, w, b


@pytest.mark.parametrize("batch", [1, 3, 17])
@pytest.mark.parametrize("n", [8, 2040, 2056])
def test_rmsnorm_matrix(ops, n, batch):
    x, w, _ = _norm_inputs(n, batch)
    buf = _padded(batch * n)
    ops.rmsnorm(buf[:batch * n].view(batch, n), x.to(DEV), w.to(DEV), EPS)
    _check_flat(buf, batch * n, R.rmsnorm_ref(x, w), n,
                f"rmsnorm n={n} B={batch}")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n", [8, 2040, 2056])
def test_layernorm_matrix(ops, n, bias):
    x, w, b = _norm_inputs(n, 1)
    buf = _padded(n)
    ops.layernorm(buf[:n], x[0].to(DEV), w.to(DEV),
                  b.to(DEV) if bias else None, EPS)
    _check_flat(buf, n, R.layernorm_ref(x[0], w, b if bias else None), n,
                f"layernorm n={n} bias={bias}")


@pytest.mark.parametrize("n,gelu,alias", [
    (8, False, False), (8, True, True), (2056, False, True),
    (2056, True, False),
    (8 * 256 * 4096 + 8, False, True),   # past the 4096-block cap
])
def test_swiglu_mul_matrix(ops, n, gelu, alias):
    g = torch.Generator().manual_seed(n + gelu)
    a = (torch.randn(n, generator=g) * 2).to(BF)
    u = torch.randn(n, generator=g).to(BF)
    r = R.swiglu_mul_ref(a, u, gelu)
    buf = _padded(n)
    if alias:
        buf[:n] = u.to(DEV)
        ops.swiglu_mul(buf[:n], a.to(DEV), buf[:n], gelu)
    else:
        ops.swiglu_mul(buf[:n], a.to(DEV), u.to(DEV), gelu)
    _check_flat(buf, n, r, 1, f"swiglu_mul n={n} gelu={gelu} alias={alias}")


# ---------------------------------------------------------------------------
# MDI_GEMV_PRE=1: the flag is latched in a static, so one fresh process
_PRE_CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import torch
import gemv_reference as R
from mdi_llm_amd.ops import require_hip_ops
ops = require_hip_ops()
bad = 0
want = dict(zip((512, 4096, 4608, 520),
                (("direct_pre", 8), ("direct_pre", 8), ("direct_pre", 16),
                 ("direct", 2))))
for case in R.PRE_CASES:
    d = case.dispatch(pre=True)
    assert (d.kernel, d.unr) == want[case.K], (case.K, d)
    inp = R.make_inputs(case)
    ref = R.reference(case, inp, pre=True)
    buf = R.run_case(ops, case, inp, "cuda:0")
    torch.cuda.synchronize()
    ok, worst, msg = R.check_out_buffer(buf, case.M, ref, case.K)
    print(f"{{case.id}} [{{d.kernel}}]: max err/bound = {{worst:.3f}} {{msg}}")
    bad += not ok
sys.exit(1 if bad else 0)
"""


def test_gemv_pre_kernel_child_process():
    tests = Path(__file__).resolve().parent
    code = _PRE_CHILD.format(tests=str(tests), root=str(tests.parent))
    env = dict(os.environ, MDI_GEMV_PRE="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, timeout=240,
                       capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count("[direct_pre]") == 3
    assert p.stdout.count("[direct]") == 1


# ---------------------------------------------------------------------------
# host guards: each refusal is a RuntimeError raised before any launch (the
# output keeps its sentinel).  swiglu-Wu-size, fp8-wscale-size and the two
# rmsnorm size cases hit checks older than the rest; they are here so that
# the list covers every argument of every op.  Mis-sized arguments are LARGER than required,
# so a missing guard could only have read valid memory.
def _t(*shape, dtype=BF):
    return torch.ones(*shape, dtype=dtype, device=DEV)


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8, device=DEV)


def _guard_calls(ops):
    M, K = 8, 32
    big = 32784   # K*2 bytes of staged x exceed 64 KiB; a multiple of 16
    W, x = _t(M, K), _t(K)
    Wq, sc = _u8(M, K), _t(M, dtype=torch.float32)
    e0 = torch.zeros(0, dtype=torch.int32, device=DEV)
    f0 = torch.zeros(0, dtype=torch.float32, device=DEV)
    e1 = torch.zeros(1, dtype=torch.int32, device=DEV)

    def gemv(o, **kw):
        a = dict(W=W, x=x, bias=None, res=None, epilogue=0, norm_w=None,
                 norm_b=None, norm_kind=0, eps=EPS, rows=1, eidx=None,
                 estride=0)
        a.update(kw)
        ops.gemv(o, **a)

    def fp8(o, **kw):
        a = dict(W=Wq, wscale=sc, x=x, bias=None, res=None, epilogue=0,
                 norm_w=None, norm_b=None, norm_kind=0, eps=EPS, rows=1)
        a.update(kw)
        ops.gemv_fp8(o, **a)

    def sw(o, **kw):
        a = dict(Wg=W, Wu=W, x=x, gelu_gate=False, norm_w=None, norm_b=None,
                 norm_kind=0, eps=EPS, eidx=None, estride=0, escale=None)
        a.update(kw)
        ops.gemv_swiglu(o, **a)

    def sw8(o, **kw):
        a = dict(Wg=Wq, gscale=sc, Wu=Wq, uscale=sc, x=x, gelu_gate=False,
                 norm_w=None, norm_b=None, norm_kind=0, eps=EPS)
        a.update(kw)
        ops.gemv_swiglu_fp8(o, **a)

    sc8 = _t(M + 8, dtype=torch.float32)
    calls = {
        "gemv-norm_w-none": lambda o: gemv(o, norm_kind=1),
        "gemv-norm_w-size": lambda o: gemv(o, norm_kind=1, norm_w=_t(K + 8)),
        "gemv-norm_b-size": lambda o: gemv(o, norm_kind=2, norm_w=_t(K),
                                           norm_b=_t(K + 8)),
        "gemv-bias-size": lambda o: gemv(o, bias=_t(M + 8)),
        "gemv-res-size": lambda o: gemv(o, res=_t(M + 8), epilogue=1),
        "gemv-K-zero": lambda o: gemv(o, x=_t(0), W=_t(0)),
        "gemv-epilogue-range": lambda o: gemv(o, epilogue=4),
        "gemv-norm_kind-range": lambda o: gemv(o, norm_kind=3, norm_w=_t(K)),
        "gemv-eidx-empty": lambda o: gemv(o, eidx=e0, estride=M * K),
        "gemv-lds": lambda o: gemv(o, W=_t(M, big), x=_t(big), norm_kind=2,
                                   norm_w=_t(big)),
        "swiglu-norm_w-none": lambda o: sw(o, norm_kind=1),
        "swiglu-norm_w-size": lambda o: sw(o, norm_kind=1, norm_w=_t(K + 8)),
        "swiglu-norm_b-size": lambda o: sw(o, norm_kind=2, norm_w=_t(K),
                                           norm_b=_t(K + 8)),
        "swiglu-Wu-size": lambda o: sw(o, Wu=_t(M + 1, K)),
        "swiglu-eidx-empty": lambda o: sw(o, eidx=e0, estride=M * K),
        "swiglu-escale-empty": lambda o: sw(o, eidx=e1, estride=M * K,
                                            escale=f0),
        "swiglu-lds": lambda o: sw(o, Wg=_t(M, big), Wu=_t(M, big),
                                   x=_t(big)),
        "fp8-norm_w-none": lambda o: fp8(o, norm_kind=1),
        "fp8-norm_w-size": lambda o: fp8(o, norm_kind=1, norm_w=_t(K + 16)),
        "fp8-norm_b-size": lambda o: fp8(o, norm_kind=2, norm_w=_t(K),
                                         norm_b=_t(K + 16)),
        "fp8-bias-size": lambda o: fp8(o, bias=_t(M + 8)),
        "fp8-res-size": lambda o: fp8(o, res=_t(M + 8), epilogue=1),
        "fp8-wscale-size": lambda o: fp8(o, wscale=sc8),
        "fp8-lds": lambda o: fp8(o, W=_u8(M, big), x=_t(big)),
        "swiglu_fp8-norm_w-none": lambda o: sw8(o, norm_kind=1),
        "swiglu_fp8-norm_w-size": lambda o: sw8(o, norm_kind=2,
                                                norm_w=_t(K + 16)),
        "swiglu_fp8-Wg-size": lambda o: sw8(o, Wg=_u8(M + 1, K)),
        "swiglu_fp8-Wu-size": lambda o: sw8(o, Wu=_u8(M + 1, K)),
        "swiglu_fp8-gscale-size": lambda o: sw8(o, gscale=sc8),
        "swiglu_fp8-uscale-size": lambda o: sw8(o, uscale=sc8),
        "swiglu_fp8-Wg-device": lambda o: sw8(o, Wg=Wq.cpu()),
        "swiglu_fp8-Wu-strided": lambda o: sw8(o, Wu=_u8(M, 2 * K)[:, :K]),
        "swiglu_fp8-lds": lambda o: sw8(o, Wg=_u8(M, big), Wu=_u8(M, big),
                                        x=_t(big)),
        # (out is the fixture's M rows inside M + PAD_ROWS valid ones, so
        # twice M elements would still land in the observed buffer)
        "rmsnorm-out-size": lambda o: ops.rmsnorm(o, _t(2, M), _t(M), EPS),
        "rmsnorm-x-ragged": lambda o: ops.rmsnorm(o, _t(M), _t(16), EPS),
        "rmsnorm-w-empty": lambda o: ops.rmsnorm(o, _t(M), _t(0), EPS),
        "layernorm-w-size": lambda o: ops.layernorm(o, _t(M), _t(M + 8),
                                                    None, EPS),
        "layernorm-b-size": lambda o: ops.layernorm(o, _t(M), _t(M),
                                                    _t(M + 8), EPS),
        "layernorm-out-size": lambda o: ops.layernorm(o, _t(2 * M),
                                                      _t(2 * M), None, EPS),
    }
    return M, calls


GUARDS = ["gemv-norm_w-none", "gemv-norm_w-size", "gemv-norm_b-size",
          "gemv-bias-size", "gemv-res-size", "gemv-K-zero",
          "gemv-epilogue-range", "gemv-norm_kind-range", "gemv-eidx-empty",
          "gemv-lds", "swiglu-norm_w-none", "swiglu-norm_w-size",
          "swiglu-norm_b-size", "swiglu-Wu-size", "swiglu-eidx-empty",
          "swiglu-escale-empty", "swiglu-lds", "fp8-norm_w-none",
          "fp8-norm_w-size", "fp8-norm_b-size", "fp8-bias-size",
          "fp8-res-size", "fp8-wscale-size", "fp8-lds",
          "swiglu_fp8-norm_w-none", "swiglu_fp8-norm_w-size",
          "swiglu_fp8-Wg-size", "swiglu_fp8-Wu-size",
          "swiglu_fp8-gscale-size", "swiglu_fp8-uscale-size",
          "swiglu_fp8-Wg-device", "swiglu_fp8-Wu-strided", "swiglu_fp8-lds",
          "rmsnorm-out-size", "rmsnorm-x-ragged", "rmsnorm-w-empty",
          "layernorm-w-size",
          "layernorm-b-size", "layernorm-out-size"]


@pytest.mark.parametrize("which", GUARDS)
def test_host_guard_refuses_before_launch(ops, which):
    M, calls = _guard_calls(ops)
    assert set(calls) == set(GUARDS)
    buf = R.new_out_buffer(M, DEV)
    with pytest.raises(RuntimeError):
        calls[which](buf[:M])
    torch.cuda.synchronize()
    assert bool((buf.float() == SENTINEL).all()), "something was launched"


def test_empty_output_is_refused(ops):
    """M == 0: the grid would be empty (an invalid launch)."""
    o = torch.empty(0, dtype=BF, device=DEV)
    x = _t(32)
    with pytest.raises(RuntimeError):
        ops.gemv(o, _t(0), x, None, None, 0)
    with pytest.raises(RuntimeError):
        ops.gemv_swiglu(o, _t(0), _t(0), x, False)
    with pytest.raises(RuntimeError):
        ops.gemv_fp8(o, _u8(0), _t(0, dtype=torch.float32), x, None, None, 0)
    with pytest.raises(RuntimeError):
        ops.gemv_swiglu_fp8(o, _u8(0), _t(0, dtype=torch.float32), _u8(0),
                            _t(0, dtype=torch.float32), x, False)


def test_int4_refuses_out_of_range_selectors(ops):
    """An epilogue or norm_kind outside its range raises for int4 as for
    bf16 and fp8 (it used to run as 0), before any launch."""
    M, K = 8, 32
    Wq, qp, x, nw = _u8(M, 64), _t(M, 1, 2), _t(K), _t(K)
    buf = R.new_out_buffer(M, DEV)
    o = buf[:M]
    with pytest.raises(RuntimeError):
        ops.gemv_int4(o, Wq, qp, x, None, None, 4)
    with pytest.raises(RuntimeError):
        ops.gemv_int4(o, Wq, qp, x, None, None, 0, nw, None, 3)
    with pytest.raises(RuntimeError):
        ops.gemv_swiglu_int4(o, Wq, qp, Wq, qp, x, False, nw, None, 3)
    torch.cuda.synchronize()
    assert bool((buf.float() == SENTINEL).all()), "something was launched"
