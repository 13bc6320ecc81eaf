"""CPU: tests/attn_fp64.py, the reference of test_gpu_attn_edges.py.
  1. the restatement equals torch.softmax-based fp64 attention on every shape the GPU file launches, in both operand forms;
  2. the exact family is exact: its operands are numbers of both 16-bit formats, and the REPLAY of the kernels' order of operations in fp32
     (tiles of 32 keys, deferred wave-uniform rescale, p rounded for P.V and unrounded in l, the combine of key splits) gives the fp64 result
     bit for bit at every key split -- and the family holds what makes it worth running: rescales taken with alpha a power of two below 1,
     rescales deferred with p up to 2^7, maxima in the last (partial) tile, splits with different partial maxima;
  3. the comparisons are sensitive: each mutation (attn_fp64.attention_fp64 / replay, `mutate=`) changes the expected bits of the exact
     family and exceeds the bound 0.5 ulp16 + slack on every case of the random family it applies to.  One cannot do both, by construction:
       l_from_rounded_p   changes nothing on the exact family (every p there IS a 16-bit number: asserted).  On the random family it moves a
                          row by |l16 / l - 1|, which the slack's `mismatch` part u16 bounds from above for ANY valid count -- it cannot
                          exceed it.  What is asserted instead: the largest move reaches a quarter of u16 in every form and format, so
                          the term counts no more than four times what the kernels' choice really costs a row."""
import math

import pytest
import torch

import attn_fp64 as A

FORMATS = (torch.bfloat16, torch.float16)
FORMS = ("d512", "kv")
CASES = [(B, N) for N in A.NS for B in A.BS]
IDS = ["%dx%d" % c for c in CASES]
RESTATED = ("key_past_n", "last_key_masked", "tile_dropped", "v_column_shifted", "query_of_next_image")
REPLAYED = ("rescale_skipped", "l_from_rounded_p", "split_weight_dropped")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _applies(mu, B, N):
    if mu == "tile_dropped":
        return N >= 2                          # a single key has no tile to lose
    if mu == "query_of_next_image":
        return N > 1                           # one key: its weight is 1 whatever the query
    if mu == "split_weight_dropped":
        return A.tiles(N) >= 2
    return True


def _ks(mu, N):
    """the key split a replayed mutation needs: a rescale after a split's first tile needs several tiles in one split"""
    return A.splits_of(N)[-1] if mu == "split_weight_dropped" else 1


# ---- 1. the restatement is the operator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_torch_softmax(case):
    B, N = case
    for form in FORMS:
        q, k, v = A.random_case(B, N, form, torch.float16)
        want = torch.softmax((q @ k.transpose(1, 2)) * math.log(2.0), -1) @ v
        pitch = A.tiles(N) * A.BN + 32
        v_t = torch.full((B, A.HD, pitch), float("nan"), dtype=torch.float64)
        v_t[:, :, :N] = v.transpose(1, 2)
        got = A.attention_kv512_fp64(q, k) if form == "kv" else A.attention_d512_fp64(q, k, v_t, N)
        assert got.shape == want.shape == (B, N, A.HD)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        if form == "kv":
            assert k is v
        out, slack, mismatch = A.out_slack(q, k, v, 1, torch.float16)
        assert torch.equal(out, A.attention_fp64(q, k, v)) and bool((slack >= 0).all()) and bool((mismatch <= slack).all())


def test_random_family_carries_its_structured_rows():
    pmax = 0.0
    for B, N in CASES:
        if N < 4:
            continue
        q, k, v = A.random_case(B, N, "d512", torch.bfloat16)
        s = q @ k.transpose(1, 2)
        stairs, last, first = A.structured_rows(N)
        assert bool((s[:, last].argmax(-1) == N - 1).all()) and bool((s[:, first].argmax(-1) == 0).all())
        for row, key in ((last, N - 1), (first, 0)):
            rest = torch.cat([s[:, row, :key], s[:, row, key + 1:]], -1)
            assert float((s[:, row, key] - rest.amax(-1)).min()) > 30.0
        steps = s[:, stairs, 5::A.BN]
        assert torch.equal(steps[0], torch.tensor([0.0, 7.5, 16.0, 23.5, 32.0, 39.5][:steps.shape[1]], dtype=torch.float64))
        r = A.replay(q, k, v, torch.bfloat16)
        if steps.shape[1] >= 3:          # the second step, 8.5, is taken (both, if a neighbour forces the first)
            assert float(r["taken"][:, stairs].min()) >= 1
        assert float(r["pmax"].max()) <= 256.0          # deferred rescales: p up to 2^8, never above
        pmax = max(pmax, float(r["pmax"][:, stairs].max()))
    assert pmax > 128.0          # the 7.5 step of the staircase is deferred somewhere: p = 2^7.5


# ---- 2. the exact family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_family_is_exact_under_the_replay(case):
    B, N = case
    for form in FORMS:
        q, k, v = A.exact_case(B, N, form)
        S = A.exact_scores(B, N)
        assert torch.equal(q @ k.transpose(1, 2), S) and torch.equal(S, S.round())
        top = S.amax(-1, keepdim=True)
        w = torch.exp2(S - top)
        assert bool(((S == top) | (S <= top - 1100) | (S >= top - 7)).all())          # survivors within 7, everything else 0 in fp64 too
        assert torch.equal(torch.log2(w.sum(-1)), torch.log2(w.sum(-1)).round())      # the sum of the weights is a power of two
        want = A.attention_fp64(q, k, v)
        assert float(want.abs().max()) > 0
        for dt in FORMATS:
            for t in (q, k, v):
                assert torch.equal(t.to(dt).double(), t), "operands are not numbers of the format"
            for ks in A.splits_of(N):
                r = A.replay(q, k, v, dt, ks)
                assert torch.equal(r["value"].double(), want), (form, dt, ks)
                assert torch.equal(_bits(r["hi"]), _bits(want.to(dt)))
                assert torch.equal(_bits(r["lo"]), _bits((want - want.to(dt).double()).to(dt)))


def test_exact_family_covers_the_schedule():
    tot = {}
    for B, N in CASES:
        q, k, v = A.exact_case(B, N, "kv")
        for ks in A.splits_of(N):
            r = A.replay(q, k, v, torch.bfloat16, ks)
            for n in ("taken", "forced", "deferred", "last"):
                tot[n, ks] = tot.get((n, ks), 0) + int((r[n] > 0).sum())
            tot["pmax"] = max(tot.get("pmax", 0.0), float(r["pmax"].max()))
            hi, lo = r["hi"].double(), r["lo"].double()
            tot["inexact16"] = tot.get("inexact16", 0) + int((lo != 0).sum())
            assert int((hi != 0).sum()) * 4 > hi.numel()          # dense: not a field of zeros
    for ks in (1, 2, 3, 4):
        assert min(tot["taken", ks], tot["forced", ks], tot["deferred", ks], tot["last", ks]) >= 20, tot
    assert tot["pmax"] == 128.0 and tot["inexact16"] > 1000, tot          # the pair's lo has something to hold
    if A.tiles(161) >= 2:          # splits with different partial maxima: the weights of the combine are not all 1
        q, k, v = A.exact_case(3, 161, "kv")
        assert not torch.equal(A.replay(q, k, v, torch.bfloat16, 3, "split_weight_dropped")["value"], A.replay(q, k, v, torch.bfloat16, 3)["value"])


# ---- 3. sensitivity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", RESTATED + REPLAYED)
def test_mutation_changes_the_exact_bits(mu):
    for B, N in CASES:
        if not _applies(mu, B, N):
            continue
        for form in FORMS:
            q, k, v = A.exact_case(B, N, form)
            want = A.attention_fp64(q, k, v)
            for dt in FORMATS:
                if mu in RESTATED:
                    got = A.attention_fp64(q, k, v, mu, 0.0 if form == "kv" else A.PAD_D512).to(dt)
                else:
                    r = A.replay(q, k, v, dt, _ks(mu, N), mu)
                    got = r["hi"]
                same = torch.equal(_bits(got), _bits(want.to(dt)))
                if mu == "l_from_rounded_p":
                    assert same, "every p of the exact family is a 16-bit number: rounding it changes nothing"
                elif mu == "rescale_skipped" and A.tiles(N) < 2:
                    assert same          # one tile: nothing to rescale
                else:
                    assert not same, (mu, B, N, form, dt)


def _fails(got, exact, slack, dt):
    x = A.ratio16(got.double(), exact, slack, dt)
    return bool(torch.isnan(x).any()) or float(x.max()) >= 1.0


@pytest.mark.parametrize("dt", FORMATS, ids=("bf16", "fp16"))
@pytest.mark.parametrize("form", FORMS)
def test_mutation_exceeds_the_bound_on_the_random_family(form, dt):
    u16 = 2.0 ** -(A.fmt(dt)[0] + 1)
    seen = {mu: [] for mu in RESTATED + REPLAYED}
    move = 0.0
    for B, N in CASES:
        q, k, v = A.random_case(B, N, form, dt)
        exact, f, _ = A.slack_terms(q, k, v, dt)
        for ks in A.splits_of(N):          # the unmutated replay is inside the bound at every split: the bound is not what fails below
            slack = f(ks)
            r = A.replay(q, k, v, dt, ks)
            assert not _fails(r["hi"], exact, slack, dt)
            assert float(A.ratio_pair(r["hi"].double() + r["lo"].double(), exact, slack, dt).max()) < 1.0
        slack = f(1)
        for mu in RESTATED:
            if _applies(mu, B, N):
                seen[mu].append((N, _fails(A.attention_fp64(q, k, v, mu, 0.0 if form == "kv" else A.PAD_D512).to(dt), exact, slack, dt)))
        for mu in REPLAYED:
            if not _applies(mu, B, N):
                continue
            ks = _ks(mu, N)
            slack = f(ks)
            base, r = A.replay(q, k, v, dt, ks), A.replay(q, k, v, dt, ks, mu)
            if mu == "l_from_rounded_p":          # per row, at its largest channel: |l16 / l - 1| in units of u16
                a, b_ = base["value"].double(), r["value"].double()
                top = a.abs().argmax(-1, keepdim=True)
                rel = ((b_ - a).gather(-1, top) / a.gather(-1, top)).abs() / u16
                assert float(rel.max()) <= 1.0 + 1e-3          # a valid count bounds it
                move = max(move, float(rel.max()))
            changed = bool((base["taken"][:, ::A.WAVE_ROWS] > 0).any()) if mu == "rescale_skipped" else True
            if changed:
                seen[mu].append((N, _fails(r["hi"], exact, slack, dt)))
    for mu in RESTATED + ("rescale_skipped", "split_weight_dropped"):
        assert seen[mu] and all(f for _, f in seen[mu]), (mu, [n for n, f in seen[mu] if not f])
    assert len(seen["rescale_skipped"]) >= 4
    assert not any(f for _, f in seen["l_from_rounded_p"])
    assert move >= 0.25, move
