"""GPU: prefill_attn (v2 by default, v1 and the 32-key chunk in child
processes) and rope_prefill_append against the fp64 references of
prefill_reference.py, under their derived bounds (no tolerance is set here).

The matrix walks the v2 kernel's wave mapping (qpk 1..8: hpb, qtpb, the
remainder head group, the idle wave at hpb 3), q-tile and 64-key chunk
edges, the flip of the wave-uniform `full` shortcut, blocks with several q
tiles and divergent causal bounds, the three head sizes and three score
profiles, each with a bf16 and an fp8 cache.  Every case plants probe keys
(weight 0.02..0.5 on one row and head) at the edges and, behind each
designated row, one key that a leaking mask would hand nearly all the
weight; test_prefill_reference_cpu.py shows on the CPU which mistakes that
catches.  Outputs are views of sentinel-padded buffers, and every input
must come back bit-unchanged.

Each case prints PREFILL_RATIO <case> <err/bound>;
profiles/prefill_error_margins.md keeps the per-family figures of one run.
"""

import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import prefill_reference as P
from attn_reference import (attn_decode_reference, attn_error_bound,
                            bf16_ulp_distance, fp8_decode, rope_tables)
from prefill_reference import C_V2, F64, SENTINEL

pytestmark = pytest.mark.gpu

if os.environ.get("MDI_PREFILL_V1") or os.environ.get("MDI_PREFILL_KCH"):
    pytest.skip("MDI_PREFILL_V1 / MDI_PREFILL_KCH change the kernel this "
                "module assumes", allow_module_level=True)

DEV = "cuda:0"
BF = torch.bfloat16
MATRIX = P.prefill_matrix()
ROPE = P.rope_matrix()


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATRIX))
def test_prefill_matrix(ops, name):
    case = P.make_prefill_case(**MATRIX[name])
    ref = case.reference()
    assert case.probes_ok(ref), (case.probe_weights(ref),
                                 case.leak_margins())
    buf, dev = P.run_prefill(ops, case, DEV)
    torch.cuda.synchronize()
    ok, ratio, msg = P.check_prefill(case, ref, buf, dev, C_V2)
    print(f"PREFILL_RATIO {name} {ratio:.4f}")
    assert ok, f"{name}: {msg}"


# ---------------------------------------------------------------------------
# MDI_PREFILL_V1 / MDI_PREFILL_KCH are latched in statics: one fresh
# process each
_CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import torch
import prefill_reference as P
from mdi_llm_amd.ops import require_hip_ops
ops = require_hip_ops()
which = {which!r}
if which == "v1":
    full = P.prefill_matrix()
    cases, c = {{n: full[n] for n in P.V1_NAMES}}, P.C_V1
else:
    cases, c = P.kch32_matrix(), P.C_V2
bad = 0
for name, kw in cases.items():
    case = P.make_prefill_case(**kw)
    ref = case.reference()
    assert case.probes_ok(ref), name
    buf, dev = P.run_prefill(ops, case, "cuda:0")
    torch.cuda.synchronize()
    ok, ratio, msg = P.check_prefill(case, ref, buf, dev, c)
    print(f"PREFILL_RATIO {{which}} {{name}} {{ratio:.4f}} {{msg}}")
    bad += not ok
sys.exit(1 if bad else 0)
"""


def _child(which, env_extra, n_cases):
    tests = Path(__file__).resolve().parent
    code = _CHILD.format(tests=str(tests), root=str(tests.parent),
                         which=which)
    p = subprocess.run([sys.executable, "-c", code],
                       env=dict(os.environ, **env_extra), timeout=240,
                       capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert p.stdout.count("PREFILL_RATIO") == n_cases


def test_prefill_v1_child_process():
    """prefill_attn_kernel under its own (fp32 P) bound.  The qpk 1, T 130
    case has waves of one block looping over 1..4 key tiles."""
    _child("v1", {"MDI_PREFILL_V1": "1"}, len(P.V1_NAMES))


def test_prefill_kch32_child_process():
    _child("kch32", {"MDI_PREFILL_KCH": "32"}, len(P.kch32_matrix()))


# ---------------------------------------------------------------------------
# rope_prefill_append
U8_SENTINEL = 0xA5
SCALE_SENTINEL = -7.0


def _pools(n_kv, max_seq, hs, kv8):
    shape = (P.N_SLOTS, P.N_LAYERS, n_kv, max_seq, hs)
    if kv8:
        return (torch.full(shape, U8_SENTINEL, dtype=torch.uint8, device=DEV),
                torch.full(shape, U8_SENTINEL, dtype=torch.uint8, device=DEV),
                torch.full(shape[:-1], SCALE_SENTINEL, device=DEV),
                torch.full(shape[:-1], SCALE_SENTINEL, device=DEV))
    return (torch.full(shape, SENTINEL, dtype=BF, device=DEV),
            torch.full(shape, SENTINEL, dtype=BF, device=DEV), None, None)


def _padded_qkv(qkv):
    n = qkv.numel()
    buf = torch.full((n + P.PAD,), SENTINEL, dtype=BF, device=DEV)
    buf[:n] = qkv.to(DEV).flatten()
    return buf, buf[:n].view(qkv.shape)


def _check_rope_and_append(raw, got, pools, cos, sin, pos0, slot, layer,
                           n_kv, hs):
    """raw/got: host bf16 [T, qkv_dim] before and after; pools: the four
    host tensors after.  Asserts the roped rows, the appended rows and that
    nothing else in the pools was written."""
    T = raw.shape[0]
    ne = cos.shape[1]
    ref = P.rope_append_reference(raw, cos, sin, pos0, n_kv, hs)
    want = ref.to(torch.float32).to(BF)
    g4 = got.reshape(T, n_kv, -1, hs)
    r4 = raw.reshape(T, n_kv, -1, hs)
    d = bf16_ulp_distance(g4[:, :, :-1], want[:, :, :-1])
    assert int(d.max()) <= 1, f"roped q/k off by {int(d.max())} bf16 ulp"
    assert torch.equal(g4[:, :, -1], r4[:, :, -1]), "a v row was changed"
    assert torch.equal(g4[..., ne:], r4[..., ne:]), \
        "a dim >= rope_ne was changed"
    kpool, vpool, kscale, vscale = pools
    rows = (slot, layer, slice(None), slice(pos0, pos0 + T))
    k_src = g4[:, :, -2].transpose(0, 1)     # [n_kv, T, hs], kernel's own
    v_src = r4[:, :, -1].transpose(0, 1)
    if kscale is None:
        assert torch.equal(kpool[rows], k_src), "appended K != roped k row"
        assert torch.equal(vpool[rows], v_src), "appended V != raw v"
    else:
        for nm, pool, tbl, src in (("K", kpool, kscale, k_src),
                                   ("V", vpool, vscale, v_src)):
            src = src.to(F64)
            sc = tbl[rows].to(F64)
            want_sc = src.abs().amax(-1).clamp_min(1e-12) / 448.0
            assert torch.allclose(sc, want_sc, rtol=1e-6, atol=0), \
                f"{nm} scale is not absmax/448 of the kernel's bf16 row"
            deq = fp8_decode(pool[rows]).to(F64) * sc[..., None]
            tol = 2.0 ** -4 * src.abs() + sc[..., None] * 2.0 ** -10
            assert bool(((deq - src).abs() <= tol).all()), \
                f"appended fp8 {nm} row outside the e4m3 half-ulp"
            zero = src.abs().amax(-1) == 0
            assert bool((pool[rows][zero] == 0).all()), \
                f"a zero {nm} row did not quantise to zero bytes"
    fills = (U8_SENTINEL, U8_SENTINEL, SCALE_SENTINEL, SCALE_SENTINEL) \
        if kscale is not None else (SENTINEL, SENTINEL, None, None)
    for t, fill in zip(pools, fills):
        if t is None:
            continue
        rest = t.clone().float()
        rest[rows] = fill
        assert bool((rest == fill).all()), \
            "an element outside [slot, layer, :, pos0:pos0+T] was written"


@pytest.mark.parametrize("name", list(ROPE))
def test_rope_prefill_append(ops, name):
    case = P.make_rope_case(**ROPE[name])
    buf, qkv = _padded_qkv(case.qkv)
    pools = _pools(case.n_kv, case.max_seq, case.hs, case.kv8)
    ops.rope_prefill_append(qkv, pools[0], pools[1], case.cos.to(DEV),
                            case.sin.to(DEV), case.pos0, case.slot,
                            case.layer, kscale=pools[2], vscale=pools[3])
    torch.cuda.synchronize()
    host = buf.cpu()
    n = case.qkv.numel()
    assert bool((host[n:].float() == SENTINEL).all()), \
        "the guard tail behind qkv was written"
    hp = [None if t is None else t.cpu() for t in pools]
    _check_rope_and_append(case.qkv, host[:n].view(case.qkv.shape), hp,
                           case.cos, case.sin, case.pos0, case.slot,
                           case.layer, case.n_kv, case.hs)
    if case.kv8:   # the all-zero v row
        zt, zg = case.zero_v
        at = (case.slot, case.layer, zg, case.pos0 + zt)
        assert float(hp[3][at]) == pytest.approx(1e-12 / 448.0, rel=1e-6)
        assert bool((hp[1][at] == 0).all())


# ---------------------------------------------------------------------------
# hand-off: rope_prefill_append -> prefill_attn -> attn_decode
HO = dict(qpk=4, n_kv=2, hs=128, max_seq=128, T1=21, T2=20)


def _prefill_steps(ops, raw, pools, cos, sin, steps, scale):
    """rope_prefill_append + prefill_attn over consecutive row ranges of
    raw; returns (roped qkv host, out host) concatenated over the steps."""
    qpk, n_kv, hs = HO["qpk"], HO["n_kv"], HO["hs"]
    roped, outs = [], []
    for a, b in steps:
        buf, qkv = _padded_qkv(raw[a:b])
        n_out = (b - a) * n_kv * qpk * hs
        obuf = torch.full((n_out + P.PAD,), SENTINEL, dtype=BF, device=DEV)
        ops.rope_prefill_append(qkv, pools[0], pools[1], cos, sin, a, P.SLOT,
                                P.LAYER, kscale=pools[2], vscale=pools[3])
        ops.prefill_attn(obuf[:n_out].view(b - a, -1), qkv, pools[0],
                         pools[1], a, P.SLOT, P.LAYER, scale,
                         kscale=pools[2], vscale=pools[3])
        torch.cuda.synchronize()
        assert bool((buf[qkv.numel():].float() == SENTINEL).all())
        assert bool((obuf[n_out:].float() == SENTINEL).all())
        roped.append(qkv.cpu())
        outs.append(obuf[:n_out].cpu().view(b - a, n_kv * qpk, hs))
    return torch.cat(roped), torch.cat(outs)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_prefill_handoff(ops, kv8):
    """The reference of each attention is taken over the cache and roped
    qkv that rope_prefill_append left, after that state itself is checked
    against the fp64 rope with the criteria of the rope matrix."""
    qpk, n_kv, hs, max_seq = HO["qpk"], HO["n_kv"], HO["hs"], HO["max_seq"]
    T1, T2 = HO["T1"], HO["T2"]
    T = T1 + T2
    scale = hs ** -0.5
    gen = torch.Generator().manual_seed(77 + kv8)
    raw = torch.randn(T + 1, n_kv * (qpk + 2) * hs, generator=gen).to(BF)
    cos, sin = rope_tables(max_seq, hs)
    cd, sd = cos.to(DEV), sin.to(DEV)

    def host(pools):
        return [None if t is None else t.cpu() for t in pools]

    # one prefill of T rows
    pa = _pools(n_kv, max_seq, hs, kv8)
    roped_a, out_a = _prefill_steps(ops, raw[:T], pa, cd, sd, [(0, T)],
                                    scale)
    ha = host(pa)
    _check_rope_and_append(raw[:T], roped_a, ha, cos, sin, 0, P.SLOT,
                           P.LAYER, n_kv, hs)
    ref = P.prefill_reference(roped_a, ha[0], ha[1], 0, P.SLOT, P.LAYER,
                              scale, ha[2], ha[3])
    r_a = P.prefill_error_ratio(out_a, ref.out, ref.A, C_V2)
    # T1 rows, then T2 rows at pos0 = T1
    pb = _pools(n_kv, max_seq, hs, kv8)
    roped_b, out_b = _prefill_steps(ops, raw[:T], pb, cd, sd,
                                    [(0, T1), (T1, T)], scale)
    r_b = P.prefill_error_ratio(out_b, ref.out, ref.A, C_V2)
    print(f"PREFILL_RATIO handoff-{'fp8' if kv8 else 'bf16'} one {r_a:.4f} "
          f"split {r_b:.4f}")
    assert r_a <= 1.0 and r_b <= 1.0
    assert torch.equal(roped_a, roped_b)
    for ta, tb in zip(ha, host(pb)):
        assert ta is None or torch.equal(ta, tb), \
            "two prefills left another cache than one"

    # decode at position T off that cache
    n = n_kv * qpk * hs
    n_chunks = 8
    dbuf = torch.full((n + P.PAD,), SENTINEL, dtype=BF, device=DEV)
    part_o = torch.full((n * n_chunks,), float("nan"), device=DEV)
    part_ml = torch.full((n_kv * qpk * n_chunks * 2,), float("nan"),
                         device=DEV)
    i32 = dict(device=DEV, dtype=torch.int32)
    ops.attn_decode(dbuf[:n], part_o, part_ml, raw[T].to(DEV), pa[0], pa[1],
                    cd, sd, torch.tensor([T], **i32),
                    torch.tensor([P.SLOT], **i32), P.LAYER, n_chunks, scale,
                    n_batch=0, kscale=pa[2], vscale=pa[3], force_split=0)
    torch.cuda.synchronize()
    assert bool((dbuf[n:].float() == SENTINEL).all())
    dec = dbuf[:n].cpu().to(F64).view(n_kv * qpk, hs)
    dref = attn_decode_reference(raw[T], ha[0], ha[1], cos, sin, T, P.SLOT,
                                 P.LAYER, scale, ha[2], ha[3])
    d_bound = attn_error_bound(dref.out, dref.A)
    assert bool(((dec - dref.out).abs() <= d_bound).all()), \
        float(((dec - dref.out).abs() / d_bound).max())

    # ... and the last row of a prefill of T + 1 rows says the same
    pc = _pools(n_kv, max_seq, hs, kv8)
    roped_c, out_c = _prefill_steps(ops, raw, pc, cd, sd, [(0, T + 1)],
                                    scale)
    hc = host(pc)
    cref = P.prefill_reference(roped_c, hc[0], hc[1], 0, P.SLOT, P.LAYER,
                               scale, hc[2], hc[3])
    assert P.prefill_error_ok(out_c, cref.out, cref.A, C_V2)
    both = d_bound + P.prefill_bound(cref.out[T], cref.A[T], C_V2)
    if kv8:
        # attn_decode attends to the current token's k/v as computed (bf16)
        # and only then stores them as fp8; a prefill reads that row back
        # from the fp8 cache.  The two exact references differ by that
        # quantisation (by itself up to 1.13x the summed bounds on these
        # inputs, measured on the CPU), so their fp64 distance is allowed
        # on top.  With a bf16 cache nothing is added.
        both = both + (dref.out - cref.out[T]).abs()
    diff = (dec - out_c[T].to(F64)).abs()
    assert bool((diff <= both).all()), float((diff / both).max())


# ---------------------------------------------------------------------------
# host guards: each refusal is raised before any launch (out, qkv and the
# pools keep their sentinels)
def _guard_args(kv8):
    qpk, n_kv, hs, max_seq, T = 2, 2, 64, 32, 4
    pools = _pools(n_kv, max_seq, hs, kv8)
    qkv = torch.full((T, n_kv * (qpk + 2) * hs), SENTINEL, dtype=BF,
                     device=DEV)
    out = torch.full((T, n_kv * qpk * hs), SENTINEL, dtype=BF, device=DEV)
    cos, sin = (t.to(DEV) for t in rope_tables(max_seq, hs))
    return dict(out=out, qkv=qkv, kpool=pools[0], vpool=pools[1],
                kscale=pools[2], vscale=pools[3], cos=cos, sin=sin, pos0=3,
                slot=1, layer=1)


def _call(ops, op, a):
    if op == "attn":
        ops.prefill_attn(a["out"], a["qkv"], a["kpool"], a["vpool"],
                         a["pos0"], a["slot"], a["layer"], 0.125,
                         kscale=a["kscale"], vscale=a["vscale"])
    else:
        ops.rope_prefill_append(a["qkv"], a["kpool"], a["vpool"], a["cos"],
                                a["sin"], a["pos0"], a["slot"], a["layer"],
                                kscale=a["kscale"], vscale=a["vscale"])


def _f32(*shape):
    return torch.full(shape, SCALE_SENTINEL, device=DEV)


# name -> (kv8, edit of the argument dict); mis-sized arguments are larger
# than required wherever that is possible
SHARED_GUARDS = {
    "pool-4d": (False, lambda a: a.update(kpool=a["kpool"][0],
                                          vpool=a["vpool"][0])),
    "pool-strided": (False, lambda a: a.update(
        kpool=a["kpool"][..., :32], vpool=a["vpool"][..., :32])),
    "pool-shapes-differ": (False, lambda a: a.update(
        vpool=torch.cat([a["vpool"], a["vpool"]], dim=3))),
    "scale-one-only": (True, lambda a: a.update(vscale=None)),
    "scale-shape": (True, lambda a: a.update(
        kscale=_f32(P.N_SLOTS, P.N_LAYERS, 2, 64))),
    "qkv-1d": (False, lambda a: a.update(qkv=a["qkv"].flatten())),
    "qkv-strided": (False, lambda a: a.update(
        qkv=torch.cat([a["qkv"], a["qkv"]], dim=1)[:, :512])),
    "qkv-width": (False, lambda a: a.update(
        qkv=torch.cat([a["qkv"], a["qkv"][:, :8]], dim=1).contiguous())),
    "qkv-qpk0": (False, lambda a: a.update(
        qkv=a["qkv"][:, :256].contiguous())),
    "T-zero": (False, lambda a: a.update(qkv=a["qkv"][:0],
                                         out=a["out"][:0])),
    "pos0-negative": (False, lambda a: a.update(pos0=-1)),
    "pos0-overflow": (False, lambda a: a.update(pos0=29)),
    "slot-range": (False, lambda a: a.update(slot=P.N_SLOTS)),
    "slot-negative": (False, lambda a: a.update(slot=-1)),
    "layer-range": (False, lambda a: a.update(layer=P.N_LAYERS)),
    "layer-negative": (False, lambda a: a.update(layer=-1)),
}
ROPE_GUARDS = {
    "cos-sin-shapes": (False, lambda a: a.update(
        sin=torch.cat([a["sin"], a["sin"]], dim=0))),
    "rope_ne-odd": (False, lambda a: a.update(
        cos=a["cos"][:, :31].contiguous(),
        sin=a["sin"][:, :31].contiguous())),
    "rope_ne-above-hs": (False, lambda a: a.update(
        cos=torch.cat([a["cos"], a["cos"]], dim=1).contiguous(),
        sin=torch.cat([a["sin"], a["sin"]], dim=1).contiguous())),
    "table-rows": (False, lambda a: a.update(
        cos=a["cos"][:6].contiguous(), sin=a["sin"][:6].contiguous())),
}
GUARDS = ([("attn", n) for n in SHARED_GUARDS]
          + [("rope", n) for n in SHARED_GUARDS]
          + [("rope", n) for n in ROPE_GUARDS])


@pytest.mark.parametrize("op,which", GUARDS)
def test_host_guard_refuses_before_launch(ops, op, which):
    kv8, edit = (SHARED_GUARDS.get(which) or ROPE_GUARDS[which])
    a = _guard_args(kv8)
    keep = dict(a)
    edit(a)
    with pytest.raises(RuntimeError):
        _call(ops, op, a)
    torch.cuda.synchronize()
    for k in ("out", "qkv", "kpool", "vpool"):
        assert bool((keep[k].float() == (U8_SENTINEL if kv8 and "pool" in k
                                         else SENTINEL)).all()), \
            f"{k} was written: something was launched"
    if kv8:
        assert bool((keep["kscale"] == SCALE_SENTINEL).all())
        assert bool((keep["vscale"] == SCALE_SENTINEL).all())


def test_guard_arguments_are_accepted_unedited(ops):
    """The unedited argument sets of the guard tests do launch: every
    refusal above is due to its one edit."""
    for kv8 in (False, True):
        for op in ("rope", "attn"):   # rope first: it fills the cache rows
            a = _guard_args(kv8)
            a["qkv"].fill_(0.5)
            a["pos0"] = 0
            if op == "attn":
                _call(ops, "rope", a)
            _call(ops, op, a)
            torch.cuda.synchronize()
            if op == "attn":
                assert bool((a["out"].float() != SENTINEL).all())
