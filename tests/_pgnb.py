"""Torch restatements of the negative-binomial PG computations: checked against the reference's recorded values on the CPU
(tests/test_pgnb_host.py), then the oracle of the NB kernels on the GPU (tests/test_gpu_pg_negative_binomial.py)."""
import torch
import torch.nn.functional as F


def expected_log_sigmoid_negative_gaussian(mean, variance, nodes, weights):
    """Per point E[log sigmoid(-f)], f ~ N(mean, max(variance, 0)), by the rule (nodes, weights): the evaluation points
    mean + sd x_q (a product, then a sum), logsigmoid, weighted, summed over q."""
    sd = torch.sqrt(variance.reshape(-1).clamp_min(0.0))
    points = mean.reshape(-1)[:, None] + sd[:, None] * nodes[None, :]
    return (F.logsigmoid(-points) * weights[None, :]).sum(dim=1).reshape(mean.shape)


def total_count_grad_terms(y, mean, variance, r, nodes, weights):
    """Per point  digamma(y + r) - digamma(r) + E[log sigmoid(-f)]: the terms of d ELBO / d r."""
    rt = torch.as_tensor(r, dtype=mean.dtype, device=mean.device)
    return (torch.special.digamma(y + rt) - torch.special.digamma(rt)
            + expected_log_sigmoid_negative_gaussian(mean, variance, nodes, weights))


def total_count_grad(y, mean, variance, r, nodes, weights):
    return torch.sum(total_count_grad_terms(y, mean, variance, r, nodes, weights))


def gauss_hermite(q, dev=None):
    from polyagamma_classification import _gauss_hermite_normal_rule
    x, w = _gauss_hermite_normal_rule(q)
    return torch.tensor(x.copy(), device=dev), torch.tensor(w.copy(), device=dev)


def nb_estep_restated(S, delta, y, r, rho, probes):
    """efgp_pg_nb_estep_update in torch: the probe sum in the kernel's order (sequential over j, no FMA), b = y + r.
    -> (mean, sigma_diag, delta after the update, residual, sum of |mean count - y|)."""
    from polyagamma_classification import _pg_omega_expectation, negative_binomial_gaussian_mean
    J = probes.shape[0]
    mean = S[0].clone()
    acc = torch.zeros_like(mean)
    for j in range(J):
        acc = acc + probes[j] * S[j + 1]
    sd = acc / torch.full_like(acc, J)                   # a true division (torch turns `/ J` into a product with 1/J)
    c = torch.sqrt((sd + mean.pow(2)).clamp_min(1e-12))
    lam = _pg_omega_expectation(c, y + r)
    dn = (delta * (1.0 - rho) + rho * lam).clamp(min=0.0)
    resid = float((dn - lam).abs().max())
    abs_err = float(torch.abs(negative_binomial_gaussian_mean(mean, sd, total_count=r) - y).sum())
    return mean, sd, dn, resid, abs_err
