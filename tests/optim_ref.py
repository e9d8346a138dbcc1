"""Float64 restatement of the tail of the reference's training iteration (models/trainer.py:188-189): the gradient clipping of
`clip_grad_norm_(parameters, max_norm)` followed by one `torch.optim.Adam` step (Kingma & Ba, with bias correction; no weight
decay, no AMSGrad).  Lists of tensors in, lists out, no torch.optim inside.  The test oracle of d3ga_amd/optim.py."""
import torch


def total_norm_ref(grads):
    """2-norm of all gradients taken together (None entries take no part)."""
    sq = [g.double().pow(2).sum() for g in grads if g is not None]
    return torch.sqrt(torch.stack(sq).sum()) if sq else torch.zeros((), dtype=torch.float64)


def clip_coef_ref(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 without clipping."""
    if max_norm is None:
        return torch.ones((), dtype=torch.float64)
    c = float(max_norm) / (norm + 1e-6)
    return torch.where(c > 1.0, torch.ones_like(c), c)          # (a NaN stays a NaN)


def clip_adam_step_ref(params, grads, exp_avg, exp_avg_sq, steps, lrs, betas, eps, max_norm):
    """One step.  params / grads / exp_avg / exp_avg_sq: lists of tensors (any float dtype; computed in float64), grads[i] None:
    tensor i is skipped entirely (no decay of its moments, its step count stays).  steps: list of ints; lrs, betas ((b1, b2)), eps:
    one per tensor.  Returns (params, exp_avg, exp_avg_sq, steps, norm) as new float64 tensors / ints; `norm` is the UNCLIPPED
    total norm (None without clipping)."""
    norm = total_norm_ref(grads) if max_norm is not None else None
    coef = clip_coef_ref(norm, max_norm)
    P, M, V, S = [], [], [], []
    for p, g, m, v, t, lr, (b1, b2), e in zip(params, grads, exp_avg, exp_avg_sq, steps, lrs, betas, eps):
        p, m, v = p.double(), m.double(), v.double()
        if g is not None:
            t = int(t) + 1
            g = coef * g.double()
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            m_hat_scale = 1.0 / (1.0 - b1 ** t)
            v_hat = v / (1.0 - b2 ** t)
            p = p - lr * m_hat_scale * m / (torch.sqrt(v_hat) + e)
        P.append(p); M.append(m); V.append(v); S.append(int(t))
    return P, M, V, S, norm


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor in and out): 2^(floor(log2 |x|) - 23), the smallest normal's for tiny x."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 23.0)


def gradient_scale(step_index, tensor_index):
    """The gradient magnitudes of the optimizer tests: on even steps 1, 10 or 100 per element (total norm far above a clip
    threshold of 2.5), on odd steps 1e-2, 1e-3 or 1e-4 (far below it for tensors of a few thousand elements): six decades."""
    k = (step_index // 2 + tensor_index) % 3
    return 10.0 ** k if step_index % 2 == 0 else 10.0 ** (-2 - k)
