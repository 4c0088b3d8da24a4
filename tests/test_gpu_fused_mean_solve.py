"""The fit's cold-start mean solve with its set-up folded into the kernel (efgp_cg_solve_mean_fused): ws evaluated in the kernel and
the operator's 48 x 48 spectrum made in its prologue, on an operator whose spectra are deferred (efgp_toeplitz_create_ex).  Everything
it writes, and everything later users of the operator compute, must be bitwise what the separate launches give."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MTOTS = (13, 17, 21, 23)


def _herm(b):
    return 0.5 * (b + torch.conj(torch.flip(b, dims=(-2, -1))))


def _system(mtot, seed, N=700):
    """Toeplitz vector of N random points on the (2 mtot - 1)^2 lag box and a Hermitian F*y (coefficients of a real function)."""
    from oracle import efgp_oracle as O
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64) * 2 - 1
    v = O.conv_vector(x, 0.4, (mtot - 1) // 2)
    fy = _herm(torch.complex(torch.randn(mtot, mtot, generator=g, dtype=torch.float64),
                             torch.randn(mtot, mtot, generator=g, dtype=torch.float64))).reshape(-1)
    return v, fy


def _weights(kind, nu, c0, ell, var, h, mtot):
    from efgp_hip.lib import lib
    from efgp_hip.ops import _stream
    ws = torch.empty(mtot * mtot, dtype=torch.complex128, device="cuda")
    rc = lib().efgp_spectral_weights(0, kind, 2, float(nu), float(ell), float(var), float(c0), float(h), int(mtot), ws.data_ptr(), None,
                                     _stream(ws.device))
    assert rc == 0
    return ws


KERNELS = [("se", 0, 0.0), ("matern12", 1, 0.5), ("matern32", 1, 1.5), ("matern52", 1, 2.5)]


@pytest.mark.parametrize("mtot", MTOTS)
@pytest.mark.parametrize("name,kind,nu", KERNELS)
def test_fused_entry_is_bitwise_the_separate_launches(mtot, name, kind, nu):
    from efgp_hip import ToeplitzOp, cg_solve, cg_solve_mean_async, cg_solve_mean_fused
    torch.cuda.set_device(0)
    v, fy = _system(mtot, 5)
    vd, fyd = v.cuda(), fy.cuda()
    ell, var, h, sig = 0.2, 1.7, 0.37 / mtot, 0.2
    c0 = (2.0 * math.pi * ell ** 2) * var if kind == 0 else var * 3.1
    centre = vd[tuple((s - 1) // 2 for s in vd.shape)].real
    ws_ref = _weights(kind, nu, c0, ell, var, h, mtot)

    op_f = ToeplitzOp(vd, defer_spectra=True)
    res = cg_solve_mean_fused(op_f, kind, nu, c0, ell, h, mtot, sig, centre, fyd, 1e-6)
    assert res is not None, "the fused entry declined a deferred 48 x 48 operator"
    beta_f, ws_f, it_f = res
    op_e = ToeplitzOp(vd)
    beta_e, it_e = cg_solve_mean_async(op_e, ws_ref, sig, centre, fyd, 1e-6)
    assert torch.equal(ws_f, ws_ref)
    assert int(it_f) == int(it_e) > 0
    assert torch.equal(beta_f, beta_e)

    # later users of the deferred operator: the 64 x 64 spectrum made on first use, the 48 x 48 one from the fused prologue
    g = torch.Generator().manual_seed(9)
    u = torch.complex(torch.randn(2, mtot * mtot, generator=g, dtype=torch.float64),
                      torch.randn(2, mtot * mtot, generator=g, dtype=torch.float64)).cuda()
    assert torch.equal(op_f.apply(u), op_e.apply(u))
    b = _herm(torch.complex(torch.randn(mtot, mtot, generator=g, dtype=torch.float64),
                            torch.randn(mtot, mtot, generator=g, dtype=torch.float64))).reshape(-1).cuda()
    diag = (700.0 * ws_ref.abs().pow(2).real + 0.25)
    outs = []
    for op in (op_f, op_e):
        x, it, _ = cg_solve(op, ws_ref, 0.25, 0, b, torch.zeros_like(b), 1e-10, max_iter=2000, early_stop=True, diag=diag,
                            batched=False, hermitian=True)
        outs.append((x, it))
    assert outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("mtot", MTOTS)
def test_deferred_operator_without_the_fused_solve(mtot):
    """A deferred operator that never meets the fused solve makes both spectra on first use: same results as an eager one."""
    from efgp_hip import ToeplitzOp, cg_solve
    v, fy = _system(mtot, 11)
    vd, fyd = v.cuda(), fy.cuda()
    ws = _weights(0, 0.0, 0.3, 0.2, 1.0, 0.4 / mtot, mtot)
    op_d, op_e = ToeplitzOp(vd, defer_spectra=True), ToeplitzOp(vd)
    outs = []
    for op in (op_d, op_e):
        x, it, _ = cg_solve(op, ws, 0.2, 0, fyd, torch.zeros_like(fyd), 1e-10, max_iter=2000, early_stop=True, diag=None,
                            batched=False, hermitian=True)
        outs.append((x, it, op.apply(fyd)))
    assert outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][2], outs[1][2])


def _model(N, seed, ell, var, eps, kern_cls="se"):
    from efgpnd import EFGPND
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 2, dtype=torch.float64, generator=g) * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1]) + 0.3 * torch.randn(N, dtype=torch.float64, generator=g)
    kern = SquaredExponential(dimension=2, init_lengthscale=ell, init_variance=var) if kern_cls == "se" else \
        Matern(dimension=2, nu=2.5, init_lengthscale=ell, init_variance=var)
    return EFGPND(x.cuda(), y.cuda(), kern, sigmasq=0.2, eps=eps, nufft_eps=1e-7, estimate_params=False,
                  opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False}), x


def _fit_and_use(model, x):
    model.fit()
    st = model._fit_state
    out = dict(beta=st["beta"].clone(), ws=st["ws"].clone(), iters=int(model.last_fit_stats["mean_cg_iters"]),
               mtot=st["mtot"])
    xn = x[:500].cuda()
    out["mean"], _ = model.predict(xn, return_variance=False)
    torch.manual_seed(3)
    _, out["var"] = model.predict(xn, variance_method="stochastic", hutchinson_probes=40)
    torch.manual_seed(4)
    out["grad"] = model.compute_gradients(trace_samples=2)
    u = torch.randn(st["ws"].numel(), dtype=torch.complex128, device="cuda")
    out["apply"] = model._toeplitz._op.apply(u)
    return out


@pytest.mark.parametrize("ell,var,eps,kern_cls", [(0.2, 2.0, 1e-4, "se"), (0.3, 1.0, 1e-4, "se"), (0.5, 1.5, 1e-3, "matern")])
def test_fit_and_its_users_match_the_unfused_fit(ell, var, eps, kern_cls, monkeypatch):
    m_f, x = _model(30000, 1, ell, var, eps, kern_cls)
    a = _fit_and_use(m_f, x)
    monkeypatch.setenv("EFGP_NO_CG_FUSED_MEAN", "1")
    m_u, _ = _model(30000, 1, ell, var, eps, kern_cls)
    b = _fit_and_use(m_u, x)
    assert a["mtot"] == b["mtot"] and a["mtot"] <= 23
    assert a["iters"] == b["iters"]
    for k in ("beta", "ws", "mean", "var", "grad", "apply"):
        assert torch.equal(a[k], b[k]), k


def test_headline_fit_is_bitwise_the_unfused_fit(monkeypatch):
    """bench.py's problem: N = 1e6, SE l = 0.2, sigma_f^2 = 2, eps 1e-4 (mtot 23): beta, the count (68) and the posterior mean."""
    import bench
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    x, y = bench.synth(1_000_000, 2, 1000, "cuda")
    outs = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("EFGP_NO_CG_FUSED_MEAN", env)
        m = EFGPND(x, y, SquaredExponential(dimension=2, init_lengthscale=bench.LS, init_variance=bench.VAR), sigmasq=bench.SIG2,
                   eps=bench.EPS, nufft_eps=bench.NUFFT_TOL, estimate_params=False,
                   opts={"cg_tolerance": bench.CG_TOL, "mean_cg_warm_start": False})
        m._compute_common_parameters(force_recompute=True)
        mean, _ = m.predict(x, return_variance=False)
        outs.append((m._fit_state["beta"].clone(), int(m.last_fit_stats["mean_cg_iters"]), mean, m.last_fit_stats["mtot"]))
    assert outs[0][3] == outs[1][3] == 23
    assert outs[0][1] == outs[1][1] == 68
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][2], outs[1][2])
