"""Host: the case builders and references of tests/_pg_edges.py (the oracle of tests/test_gpu_pg_kernel_edges.py) -- that every
special point is where the case says, that no p > 0.5 decision hangs on one rounding, how far the float64 restatement of
Lambda = b tanh(c / 2) / (2 c) sits from the function itself (mpmath, 50 digits), and what torch does with the non-finite
inputs, written out so that a change of its semantics shows here and not as a kernel failure on the GPU."""
import math

import numpy as np
import pytest
import torch

import _pg_edges as E
import _pgnb

_F = torch.float64
EPS = 2.0 ** -52


@pytest.mark.parametrize("likelihood", ["bernoulli", "negative_binomial"])
@pytest.mark.parametrize("N", E.ESTEP_SIZES)
def test_every_special_kind_is_present_at_every_size(N, likelihood):
    """A size smaller than the table holds N kinds per case; the cases of every `start` together hold them all."""
    want = E.estep_kinds(likelihood, 2, overflow=True)
    assert len(want) >= 12 and len(set(want)) == len(want)
    starts = range(0, len(want), N) if N < len(want) else [0]
    seen = {}
    for start in starts:
        c = E.estep_case(N, 2, likelihood, overflow=True, start=start)
        assert c["undecided"] == 0
        assert len(set(c["kinds"].values())) == len(c["kinds"]) == min(N, len(want))
        assert N - 1 in c["kinds"].values() or c["max_index"] == N - 1
        seen.update(c["kinds"])
    assert sorted(seen) == sorted(want)
    if N >= len(want):
        c = E.estep_case(N, 2, likelihood, overflow=True)
        (mean, sd, dn, _, _), _ = E.estep_reference(c, 0.7, r=None if likelihood == "bernoulli" else 1.0)
        k = c["kinds"]
        s = sd + mean.pow(2)
        assert mean[k["clamp_m0_sd0"]] == 0 and sd[k["clamp_m0_sd0"]] == 0
        assert s[k["sum_exactly_zero"]] == 0 and s[k["sum_negative"]] < 0
        assert s[k["c2_one_ulp_below_1e-12"]] == E.BELOW_1E12 < 1e-12 < E.ABOVE_1E12 == s[k["c2_one_ulp_above_1e-12"]]
        assert dn[k["delta0_negative"]] == 0 and c["delta0"][k["delta0_negative"]] < 0
        assert float((c["delta0"] * 0.3 + 0.7 * dn.new_tensor(2.5e5))[k["delta0_negative"]]) < 0       # negative before the clamp
        if likelihood == "bernoulli":
            for name in ("m_plus_tiny_y0", "m_minus_tiny_y1"):
                assert abs(float(mean[k[name]])) == E.TINY
            assert math.copysign(1.0, float(c["y"][k["y_minus_zero"]])) == -1.0 and c["y"][k["y_two"]] == 2.0
            assert [float(c["pg_b"][k[n]]) for n in ("b_zero", "b_tiny", "b_one", "b_1e6")] == [0.0, 1e-300, 1.0, 1e6]
        else:
            assert float(mean[k["m_710_mean_count_inf"]]) == 710.0 and c["y"][k["y_1e4"]] == 1e4


def test_special_kinds_without_probes_or_shapes():
    assert not set(E.estep_kinds("bernoulli", 0)) & set(E._NEEDS_SD)
    assert not set(E.estep_kinds("bernoulli", 2, with_b=False)) & set(E._NEEDS_B)
    c = E.estep_case(65, 0, "bernoulli")
    (_, sd, _, _, _), _ = E.estep_reference(c, 0.7)
    assert bool((sd == 0).all()) and c["S"].shape == (1, 65) and c["probes"].shape == (0, 65)


@pytest.mark.parametrize("position", E.MAX_POSITIONS)
def test_planted_maximum_sits_where_the_case_says(position):
    N = E.WRAP + 257
    want = {"index_0": 0, "wave3_last_lane": 255, "last_thread_of_last_workgroup": 262143, "wrapped_tail": N - 1}[position]
    assert E.blocks(N) == 1024 and E.max_index(position, N) == want
    for lik, r in (("bernoulli", None), ("negative_binomial", 37.5)):
        c = E.estep_case(N, 2, lik, max_at=position)
        for rho in (0.0, 0.7):
            (_, sd, dn, resid, _), _ = E.estep_reference(c, rho, r)
            from polyagamma_classification import _pg_omega_expectation
            b = (c["pg_b"] if r is None else c["y"] + r)
            lam = _pg_omega_expectation(torch.sqrt((sd + c["S"][0].pow(2)).clamp_min(1e-12)), b)
            gap = (dn - lam).abs()
            assert int(gap.argmax()) == want and float(gap[want]) == resid
            assert resid > 1e3 * float(torch.cat([gap[:want], gap[want + 1:]]).max())        # alone at the top, not one of many
        assert E.estep_reference(c, 1.0, r)[0][3] == 0.0


def test_all_hits_and_no_hits_cases():
    N = 1025
    for hits, count in ((True, N), (False, 0)):
        c = E.estep_case(N, 2, "bernoulli", all_hits=hits)
        assert E.estep_reference(c, 0.7)[0][4] == count


def test_lambda_restatement_against_mpmath():
    """Lambda(b, c) = b tanh(c / 2) / (2 c) at 50 digits against the float64 restatement, c from 1e-6 (the clamp arm: c2 = 1e-12)
    to 1.6e3: the distance at which a correct kernel may sit from the restatement."""
    mp = pytest.importorskip("mpmath")
    from polyagamma_classification import _pg_omega_expectation
    mp.mp.dps = 50
    g = torch.Generator().manual_seed(7)
    c = torch.cat([10.0 ** (torch.rand(4000, generator=g, dtype=_F) * (math.log10(1.6e3) + 6.0) - 6.0),
                   torch.tensor([1e-6, math.sqrt(E.ABOVE_1E12), 1e-3, 1.0, 36.7, 37.5, 40.0, 800.0, 1.6e3], dtype=_F)])
    worst, at = 0.0, None
    for b in (1.0, 0.7, 1e6 + 37.5):
        got = _pg_omega_expectation(c, torch.full_like(c, b)).tolist()
        for cv, gv in zip(c.tolist(), got):
            exact = mp.mpf(b) * mp.tanh(mp.mpf(cv) / 2) / (2 * mp.mpf(cv))
            ulp = float(abs(mp.mpf(gv) - exact) / exact) / EPS
            if ulp > worst:
                worst, at = ulp, (b, cv)
    print(f"\nLambda restatement against mpmath (50 digits), c in [1e-6, 1.6e3]: worst relative error {worst:.2f} ulp at b, c = {at}")
    assert worst <= 8.0                                  # four roundings and a tanh: well inside the 45 ulp (1e-14) of the GPU tests
    # the clamp arm: c2 <= 1e-12 gives c = 1e-6 whatever the sum was
    lam = _pg_omega_expectation(torch.sqrt(torch.tensor([-3.0, 0.0, E.BELOW_1E12], dtype=_F).clamp_min(1e-12)), torch.ones(3, dtype=_F))
    exact = float(mp.tanh(mp.mpf(1e-6) / 2) / (2 * mp.mpf(1e-6)))
    assert bool((lam == lam[0]).all()) and abs(float(lam[0]) - exact) <= 4 * EPS * exact


def test_saturated_tanh_arm_is_b_over_2c():
    from polyagamma_classification import _pg_omega_expectation
    for m in (40.0, 800.0):
        c = torch.tensor([math.sqrt(0.3 + m * m)], dtype=_F)
        assert float(_pg_omega_expectation(c, torch.tensor([3.0], dtype=_F))) == 0.5 * 3.0 / float(c)


# ---- what torch does with NaN and inf: the rule the kernels are held to ---------------------------------------------------------
def test_torch_clamp_max_and_where_keep_nan():
    nan = torch.tensor([float("nan")], dtype=_F)
    assert math.isnan(float(nan.clamp_min(0.0))) and math.isnan(float(nan.clamp(min=0.0)))
    assert math.isnan(float(torch.tensor([1.0, float("nan"), 3.0], dtype=_F).abs().max()))
    assert float(torch.where(nan > 1e-8, torch.tensor([9.0], dtype=_F), torch.tensor([0.25], dtype=_F))) == 0.25
    assert not bool(torch.sigmoid(nan).gt(0.5))


def _planted(likelihood, what, r=None, rho=0.7):
    base = E.nonfinite_base(likelihood)
    case, at = E.plant_nonfinite(base, what)
    return base, case, at, E.estep_reference(base, rho, r), E.estep_reference(case, rho, r)


def test_nonfinite_cases_are_planted_in_the_last_workgroup():
    base = E.nonfinite_base("bernoulli")
    assert base["S"].shape[1] == E.NONFINITE_N == 257 and E.NONFINITE_AT // E.THREADS == E.blocks(257) - 1
    assert sorted(base["kinds"]) == sorted(E.estep_kinds("bernoulli")) and max(base["kinds"].values()) < 252
    for what in E.ESTEP_NONFINITE:
        _, at = E.plant_nonfinite(base, what)
        assert at == ([252, 253, 254, 255] if what == "all" else [256])


def test_restatement_on_a_nan_mean():
    base, case, (i,), ((_, _, d0, r0, c0), _), ((mean, sd, dn, resid, correct), _) = _planted("bernoulli", "nan_mean")
    assert math.isnan(float(mean[i])) and math.isfinite(float(sd[i]))
    assert float(dn[i]) == 0.7 * (0.25 * float(case["pg_b"][i]))                              # the b / 4 arm, finite
    assert int(torch.isnan(dn).sum()) == 0 and resid == r0
    assert correct == c0 - int(_hit(base, i)) + int(case["y"][i] == 0)                        # sigmoid(NaN) > 0.5 is False


def _hit(case, i):
    """Whether background point i of a clean case is a hit: mean > 0 against y != 0."""
    return bool((case["S"][0, i] > 0) == (case["y"][i] != 0))


def test_restatement_on_a_nan_sigma_diag():
    base, case, (i,), ((_, _, _, r0, c0), _), ((mean, sd, dn, resid, correct), _) = _planted("bernoulli", "nan_probe_row")
    assert float(mean[i]) == 1.0 and float(case["y"][i]) == 1.0 and math.isnan(float(sd[i]))
    assert float(dn[i]) == float(case["delta0"][i]) * (1.0 - 0.7) + 0.7 * (0.25 * float(case["pg_b"][i]))
    assert resid == r0 and int(torch.isnan(dn).sum()) == 0
    assert correct == c0 - int(_hit(base, i))                                                   # sigmoid(NaN) > 0.5 is False: a miss


def test_restatement_on_a_nan_delta0():
    base, case, (i,), (ref0, _), ((_, _, dn, resid, correct), _) = _planted("bernoulli", "nan_delta0")
    assert math.isnan(float(dn[i])) and int(torch.isnan(dn).sum()) == 1 and math.isnan(resid) and correct == ref0[4]


def test_restatement_on_an_infinite_mean():
    base, case, (i,), (ref0, _), ((mean, sd, dn, resid, correct), _) = _planted("bernoulli", "inf_mean")
    assert float(mean[i]) == math.inf and float(dn[i]) == float(case["delta0"][i]) * (1.0 - 0.7)     # Lambda = b / (2 inf) = 0
    assert resid == ref0[3] and correct == ref0[4] - int(_hit(base, i)) + int(case["y"][i] != 0)


def test_restatement_on_all_of_them():
    _, _, at, _, ((mean, sd, dn, resid, _), _) = _planted("bernoulli", "all")
    assert at == [252, 253, 254, 255] and math.isnan(resid)
    assert torch.isnan(mean).nonzero().flatten().tolist() == [252] and torch.isnan(sd).nonzero().flatten().tolist() == [253]
    assert torch.isnan(dn).nonzero().flatten().tolist() == [254] and float(mean[255]) == math.inf


@pytest.mark.parametrize("r", E.NB_TOTAL_COUNTS)
def test_negative_binomial_restatement_on_nonfinite_inputs(r):
    _, _, (i,), ((_, _, _, r0, a0), t0), ((_, sd, dn, resid, abs_err), terms) = _planted("negative_binomial", "nb_nan_sigma_diag", r)
    assert math.isnan(float(sd[i])) and math.isnan(float(terms[i])) and math.isnan(abs_err) and math.isfinite(a0)
    assert int(torch.isnan(terms).sum()) == 1 and resid == r0 and math.isfinite(float(dn[i]))
    _, _, (i,), _, ((_, _, _, _, abs_err), terms) = _planted("negative_binomial", "inf_mean", r)
    assert float(terms[i]) == math.inf and abs_err == math.inf
    # the overflow case: r exp(710.15) is +inf, and so is the sum
    c = E.estep_case(257, 2, "negative_binomial", overflow=True)
    (out, terms) = E.estep_reference(c, 0.7, r)
    assert out[4] == math.inf and float(terms[c["kinds"]["m_710_mean_count_inf"]]) == math.inf and E.fsum_terms(terms)[0] == math.inf


def test_gradient_reference_on_nonfinite_inputs_and_outside_the_digamma_domain():
    x, w = _pgnb.gauss_hermite(2)
    y, mean, sd, kinds = E.grad_case(257)
    assert len(kinds) == 5 and float(sd[kinds["y1e4_sd_negative"]]) < 0 and abs(float(mean[kinds["y0_m_plus_800"]])) == 800
    total, mag = E.grad_reference(y, mean, sd, 1.0, x, w)
    assert math.isfinite(total) and mag >= abs(total)
    for what in ("sd", "mean", "y"):
        yy, mm, ss = y.clone(), mean.clone(), sd.clone()
        {"sd": ss, "mean": mm, "y": yy}[what][256] = float("nan")
        assert math.isnan(E.grad_reference(yy, mm, ss, 1.0, x, w)[0])
    # torch's digamma continues below zero by reflection; the kernel's is defined for x > 0 only and answers NaN elsewhere
    assert math.isfinite(float(torch.special.digamma(torch.tensor(-3.5, dtype=_F))))


def test_mstep_reference_against_einsum():
    for M, J in ((1, 0), (255, 1), (257, 3)):
        bx, bj, R, dp = E.mstep_case(M, J)
        t1, t2, grad, mag1, mag2 = E.mstep_reference(bx, bj, R, dp)
        e1 = torch.einsum("kp,k->p", dp, (bx.conj() * bx).real)
        e2 = torch.einsum("jk,kp->jp", (R.conj() * bj).real, dp).mean(dim=0) if J else torch.zeros(4, dtype=_F)
        for p in range(4):
            assert abs(t1[p] - float(e1[p])) <= 1e-13 * mag1[p] and abs(t2[p] - float(e2[p])) <= 1e-13 * max(mag2[p], 1e-300)
            assert grad[p] == 0.5 * (t1[p] - t2[p]) and mag1[p] >= abs(t1[p]) and mag2[p] >= abs(t2[p])
        if J == 0:
            assert t2 == [0.0] * 4 and grad == [0.5 * v for v in t1]


def test_depth_rules():
    assert E.sum_depth(1) == 1 + 6 + 4 + 1 + 6 + 4 and E.sum_depth(E.WRAP + 1) == 2 + 6 + 4 + 4 + 6 + 4
    assert E.mstep_depth(E.WRAP + 5, 3) == (2 + 10 + 1024 + 4, 2 + 10 + 1024 + 14)
