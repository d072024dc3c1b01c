"""The float64 torch restatement of the entropy and information-gain maps (gdrf_predict_info, csrc/predict_info.h), built from
oracle.gdrf_oracle.conditional and the model's parameters exactly as tests/_mc_util.py::restate builds theta:

    mu[s,k,n] = f_loc[k,n] + mean[k,n] + f_var[k,n] eps[s,k,n];  theta_s = softmax_k(mu[s]);  p_s = theta_s Phi
    h(q) = -sum_i q_i log q_i  (0 log 0 = 0);  theta_bar = mean_s theta_s;  p_bar = theta_bar Phi

(test infrastructure; may import oracle/)."""
import torch

from tests._mc_util import restate

NAMES = ("topic_entropy", "topic_expected_entropy", "topic_information", "word_entropy", "word_expected_entropy", "word_information")
TOL = {torch.float64: 1e-9, torch.float32: 5e-4}      # the predictive path's, max-abs error over max-abs value


def entropy(q: torch.Tensor) -> torch.Tensor:
    """h over the last axis, in float64, with 0 log 0 = 0"""
    q = q.double()
    return -torch.where(q > 0, q * q.clamp_min(1e-300).log(), torch.zeros_like(q)).sum(-1)


def info_ref(m, xs, eps) -> torch.Tensor:
    """(6, n) float64, rows in the order of NAMES, of the oracle model m at rows xs under the injected draws eps (S, K, n)"""
    _, theta, _ = restate(m, xs, eps)                                       # (S, n, K)
    with torch.no_grad():
        phi = m.constrained()["phi"].double()
    tb = theta.mean(0)
    te, tx = entropy(tb), entropy(theta).mean(0)
    we, wx = entropy(tb @ phi), entropy(theta @ phi).mean(0)
    return torch.stack([te, tx, te - tx, we, wx, we - wx])


def errors(out: torch.Tensor, ref: torch.Tensor, one_word: bool = False):
    """(worst entropy error as max-abs over max-abs value, worst information error as max-abs over the largest entropy of its family).
    ``one_word`` (V = 1): every word quantity is exactly 0 and the restatement returns its own rounding of p = sum_k theta_k = 1, about
    1e-16, so an error relative to that value measures nothing; the word rows are then held to the same figure as an absolute error,
    i.e. relative to p = 1, the only term of the sum."""
    out, ref = out.double().cpu(), ref.double().cpu()
    ent, inf = 0.0, 0.0
    for base in (0, 3):
        fixed = one_word and base == 3
        top = 1.0 if fixed else float(ref[base:base + 2].abs().max())
        for i in (base, base + 1):
            ent = max(ent, float((out[i] - ref[i]).abs().max()) / (1.0 if fixed else float(ref[i].abs().max()) + 1e-300))
        inf = max(inf, float((out[base + 2] - ref[base + 2]).abs().max()) / (top + 1e-300))
    return ent, inf
