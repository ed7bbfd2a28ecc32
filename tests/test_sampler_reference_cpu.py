"""CPU: the sampler reference of sampler_reference.py is right, and every
case of its table is fit to test with.

The reference is pinned from three sides: its kept set equals what the torch
sampler of models/sampling.py keeps, its hash equals values worked out with
plain Python integers, and its draws behave as Gumbel-max draws must.  Then
every case the GPU matrix will run is checked on the reference alone: at
least 98% of its draws are decisive, its top-p margin clears delta, and each
of its perturbed references really does draw differently, so a kernel with
that defect could not pass.
"""

import math

import numpy as np
import pytest
import torch

import sampler_reference as R
from sampler_reference import (SHAPE_CASES, THRESHOLD_CASES, TIE_CASES,
                               case_logits, case_reference, code_of,
                               codes_to_bf16, draw, draw_many,
                               final_threshold, gumbel, hash_u32,
                               inv_temp_f32, perturbed_winners, salt_of,
                               sortable_codes, tie_logits, topk_threshold,
                               topp_threshold, uu_of_hash)

from mdi_llm_amd.models.sampling import logits_to_probs


# ---------------------------------------------------------------------------
# codes
def test_codes_order_is_float_order_except_signed_zero():
    vals = torch.tensor([-float("inf"), -3.0e38, -2.5, -1.0, -1e-40, -0.0,
                         0.0, 1e-40, 1.0, 2.5, 3.0e38, float("inf")]
                        ).to(torch.bfloat16)
    codes = sortable_codes(vals)
    assert (np.diff(codes) > 0).all()          # strictly increasing
    assert codes[5] == 0x7FFF and codes[6] == 0x8000   # -0 below +0
    assert torch.equal(codes_to_bf16(codes).view(torch.int16),
                       vals.view(torch.int16))


def test_codes_round_trip_every_code():
    codes = np.arange(65536)
    assert (sortable_codes(codes_to_bf16(codes)) == codes).all()
    assert code_of(8.0) == 0xC100 and code_of(-1.0) == 0x407F


# ---------------------------------------------------------------------------
# thresholds against the torch sampler
def _plain_logits():
    """1000 distinct non-zero bf16 values, in random order."""
    g = torch.Generator().manual_seed(12)
    pool = (torch.randn(8000, generator=g) * 1.5).to(torch.bfloat16)
    pool = torch.unique(pool.float())
    pool = pool[pool != 0]
    lg = pool[torch.randperm(pool.numel(), generator=g)[:1000]]
    assert torch.unique(lg).numel() == 1000
    return lg.to(torch.bfloat16)


@pytest.mark.parametrize("k,p", [(50, 1.0), (0, 0.6), (50, 0.8)],
                         ids=["top_k", "top_p", "top_k_then_top_p"])
def test_kept_set_equals_torch_sampler(k, p):
    lg = _plain_logits()
    T = 0.8
    codes = sortable_codes(lg)
    t, margin, delta = final_threshold(lg, T, k, p)
    # torch's own fp32 softmax + cumsum must not decide the boundary either
    assert margin > max(delta, 1e-5)
    assert int((codes == t).sum()) == 1        # no tie at the boundary
    want = logits_to_probs(lg, T, k if k else None, p) > 0
    got = torch.from_numpy(codes >= t)
    assert torch.equal(got, want), (int(got.sum()), int(want.sum()))
    assert 1 < int(got.sum()) < 1000


def test_ties_at_kth_value_are_all_kept():
    lg = torch.tensor([0.5, 3.0, 1.0, 2.0, 1.0, -1.0, 1.0, 0.25]
                      ).to(torch.bfloat16)
    codes = sortable_codes(lg)
    t = topk_threshold(codes, 3)
    assert t == code_of(1.0)
    assert int((codes >= t).sum()) == 5


def test_inactive_filters_keep_everything():
    lg = _plain_logits()
    codes = sortable_codes(lg)
    for k in (0, -1, 1000, 1001):
        assert topk_threshold(codes, k) == 0
    assert topk_threshold(codes, 999) == np.sort(codes)[1]
    for p in (1.0, 1.5, 0.0):
        assert topp_threshold(codes, lg, 1.0, p, 0) == (0, math.inf)
        assert final_threshold(lg, 1.0, 0, p)[0] == 0


def test_top_p_mass_is_restricted_to_top_k_set():
    # masses 0.4 0.3 0.2 0.1: alone, p = 0.75 keeps three; inside top-2
    # the fractions are 4/7 and 1, and p = 0.75 keeps two
    lg = torch.log(torch.tensor([0.4, 0.3, 0.2, 0.1])).to(torch.bfloat16)
    codes = sortable_codes(lg)
    t_alone, _ = topp_threshold(codes, lg, 1.0, 0.75, 0)
    kt = topk_threshold(codes, 2)
    t_both, _ = topp_threshold(codes, lg, 1.0, 0.75, kt)
    assert int((codes >= t_alone).sum()) == 3
    assert int((codes >= t_both).sum()) == 2
    # p tighter than k: the nucleus threshold wins the max
    t_tight, margin = topp_threshold(codes, lg, 1.0, 0.3, topk_threshold(
        codes, 3))
    assert int((codes >= t_tight).sum()) == 1
    assert margin == pytest.approx(min(0.3, 0.4 / 0.9 - 0.3), abs=2e-3)


# ---------------------------------------------------------------------------
# RNG
def _hash_int(x):
    """hash_u32 in plain Python integers, written out independently."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) % (1 << 32)
    x ^= x >> 15
    x = (x * 0x846CA68B) % (1 << 32)
    x ^= x >> 16
    return x


def test_hash_against_hand_computed_values():
    known = {0: 0, 1: 0x688990C0, 2: 0xD1132181, 0xFFFFFFFF: 0x6768824A,
             0x12345678: 0xF5E71C96}
    for x, want in known.items():
        assert _hash_int(x) == want
        assert int(hash_u32(np.array([x], dtype=np.uint32))[0]) == want
    # the salt and one full index hash of key (seed 7, pos 5, slot 3)
    salt = (7 ^ (5 * 0x9E3779B9) ^ (3 * 0x85EBCA6B)) % (1 << 32)
    assert salt == 0x86D63FDB == int(salt_of(7, 5, 3))
    h = _hash_int(_hash_int(11 ^ salt) + salt)
    assert h == 0xAC32D161
    uu = np.float32(h >> 8) * np.float32(2.0 ** -24) + np.float32(1e-12)
    g = gumbel(12, 7, 5, 3)
    assert g[11] == -math.log(-math.log(float(uu)))
    # 32-bit wraparound of the products, and of pos + pos_bias as unsigned
    assert int(salt_of(1, 1 << 20, 70000)) == (
        1 ^ ((1 << 20) * 0x9E3779B9) ^ (70000 * 0x85EBCA6B)) % (1 << 32)


def test_uu_never_reaches_zero_or_one():
    lo, hi = uu_of_hash(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert lo.dtype == np.float32
    assert 0.0 < float(lo) == float(np.float32(1e-12))
    assert float(hi) == 1.0 - 2.0 ** -24 < 1.0
    g = gumbel(1 << 20, 123, 45, 6)
    assert np.isfinite(g).all()
    assert g.min() > -3.4 and g.max() < 27.7


def test_draw_is_argmax_of_logit_plus_gumbel():
    lg = case_logits(SHAPE_CASES["V1000"])
    it = inv_temp_f32(0.8)
    for pos, slot in ((0, 0), (17, 3), (255, 9)):
        s = lg.double().numpy() * it + gumbel(1000, 7, pos, slot)
        order = np.argsort(-s, kind="stable")
        w, gap, eps = draw(lg, 0, it, True, 7, pos, slot)
        assert w == order[0]
        assert gap == pytest.approx(s[order[0]] - s[order[1]], abs=1e-12)
        assert 1e-6 < eps < 3e-5
    # restricted to a kept set
    t = topk_threshold(sortable_codes(lg), 50)
    keep = sortable_codes(lg) >= t
    s = np.where(keep, lg.double().numpy() * it + gumbel(1000, 7, 4, 2),
                 -np.inf)
    assert draw(lg, t, it, True, 7, 4, 2)[0] == int(s.argmax())


@pytest.mark.parametrize("name", list(TIE_CASES))
def test_greedy_reference_takes_lowest_index(name):
    lg = tie_logits(name)
    V, idx = TIE_CASES[name]
    assert (lg.float() == lg.float().max()).nonzero().flatten().tolist() \
        == list(idx)
    d = draw_many(lg, 0, inv_temp_f32(0.0), False, 7, [0, 1], [0, 1])
    assert d.winner.tolist() == [min(idx)] * 2
    assert d.decisive.all() and (d.gap == 0).all()
    assert min(idx) == int(torch.argmax(lg.float()))   # first occurrence


def test_every_kept_token_wins_when_noise_dominates():
    for name in ("V4096_T50_k8", "k8", "negative_k8"):
        case = R.SHAPE_CASES.get(name) or THRESHOLD_CASES[name]
        _, _, _, d = case_reference(case)
        assert d.kept.size == 8
        assert set(d.winner.tolist()) == set(d.kept.tolist())


# ---------------------------------------------------------------------------
# the case table
def test_case_table_covers_what_it_should():
    T = THRESHOLD_CASES
    for k in (1, 2, 8, 255, 256, 257):
        assert T[f"k{k}"].k == k and T[f"k{k}"].V == 4096
    for temp in (0.5, 1.0, 2.0):
        for p in (0.1, 0.5, 0.9, 0.999):
            c = T[f"p{p}_T{temp}"]
            assert (c.p, c.T, c.k, c.V) == (p, temp, 0, 4096)
    thr = {n: case_reference(c)[0] for n, c in T.items()}
    assert thr["lo_byte_00"] & 0xFF == 0x00
    assert thr["lo_byte_ff"] & 0xFF == 0xFF
    assert thr["zero_plus_is_threshold"] == 0x8000
    assert thr["zero_minus_is_threshold"] == 0x7FFF
    assert thr["negative_k8"] < 0x7F80          # a negative value
    assert (case_logits(T["negative_k8"]).float() < 0).all()
    z = sortable_codes(case_logits(T["zero_plus_is_threshold"]))
    assert (z == 0x8000).sum() == 1 and (z == 0x7FFF).sum() == 1
    assert (z > 0x8000).any() and (z < 0x7FFF).any()
    # bucket edge: 3 above the threshold's hi bucket, exactly 5 inside it
    e = sortable_codes(case_logits(T["bucket_edge"]))
    hi = thr["bucket_edge"] >> 8
    assert ((e >> 8) > hi).sum() == 3 and ((e >> 8) == hi).sum() == 5
    assert T["bucket_edge"].k == 8
    # the tie keeps more than k
    assert case_reference(T["tie_at_kth"])[3].kept.size == 10
    assert case_reference(T["dominant"])[3].kept.size == 1
    # k with p: the nucleus threshold is above the top-k one, and below
    for name, tighter in (("k4_p0.85_p_tighter", True),
                          ("k3_p0.999_k_tighter", False)):
        c = T[name]
        kt = topk_threshold(sortable_codes(case_logits(c)), c.k)
        assert (thr[name] > kt) == tighter
    assert {c.V for c in SHAPE_CASES.values()} == {1, 63, 1000, 4096, 32769,
                                                   128256}
    assert any(c.k > c.V for c in SHAPE_CASES.values())
    # the 128k top-k case keeps 201 tokens through a tie at the 200th value
    assert case_reference(SHAPE_CASES["V128256_k200"])[3].kept.size == 201


ALL_CASES = {**THRESHOLD_CASES, **SHAPE_CASES}


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_case_preconditions(name):
    """What the GPU test asserts before it trusts a case, on the CPU."""
    case = ALL_CASES[name]
    t, margin, delta, d = case_reference(case)
    n_dec = int(d.decisive.sum())
    print(f"{name}: t={t:#06x} kept={d.kept.size} draws={case.n} "
          f"min gap={d.gap.min():.3g} max eps={d.eps.max():.3g} "
          f"non-decisive={case.n - n_dec} margin={margin:.3g} "
          f"delta={delta:.3g}")
    assert n_dec >= (1 - R.MAX_NONDECISIVE) * case.n
    assert margin >= delta
    assert d.eps.max() < 2e-4
    assert (d.winner >= 0).all()


@pytest.mark.parametrize("name", list(THRESHOLD_CASES))
def test_case_has_teeth(name):
    """Each perturbed reference differs from the true one on a decisive
    draw; and a tooth is left out only where it cannot exist."""
    case = THRESHOLD_CASES[name]
    t, _, _, d = case_reference(case)
    for tooth in case.teeth:
        w = perturbed_winners(case, tooth)
        assert ((w != d.winner) & d.decisive).any(), tooth
    assert {"lower", "higher"} <= set(case.teeth)
    # one kept token: every key draws it.  Otherwise the key must bite.
    assert ("key" in case.teeth) == (d.kept.size > 1)
    # the mass restriction can only show where p is tighter than k
    kt = topk_threshold(sortable_codes(case_logits(case)), case.k)
    assert ("nomask" in case.teeth) == (case.k > 0 and case.p < 1 and t > kt)
    # the code below the threshold is occupied, or `lower` would be empty
    assert (sortable_codes(case_logits(case)) == t - 1).any()


@pytest.mark.parametrize("B", [2, 5, 16])
def test_batch_rows_preconditions(B):
    """Rows of the batched-equals-single test: distinct logits and keys,
    every top-p margin above delta, every draw decisive."""
    rows, pos, slot = R.batch_rows(B)
    assert rows.shape == (B, R.BATCH_V)
    assert len({r.numpy().view(np.int16).tobytes()
                for r in rows.view(torch.int16)}) == B
    assert len(set(pos.tolist())) == B and len(set(slot.tolist())) > 1
    for k, p in R.BATCH_MODES.values():
        for b in range(B):
            t, margin, delta = final_threshold(rows[b], R.BATCH_T, k, p)
            assert margin >= delta
            for s in (slot[b], b):
                d = draw_many(rows[b], t, inv_temp_f32(R.BATCH_T), True, 21,
                              [pos[b]], [s])
                assert d.decisive.all()
