"""Reference arithmetic of the attention rollout map, in float64 on the CPU (shared by tests/test_rollout.py and tests/test_gpu_rollout.py).

`rollout_reference`: the loop of the reference's visualiser (ecg_vit.py:184-193) on per-layer probabilities, with the COMPUTED row sums.
`rollout_closed_form`: the closed form the kernels implement -- the row sums of A + I taken as exactly 2 -- on probabilities, and
`rollout_closed_form_qkv` the same with P rebuilt from one record's own qkv rows and log-sum-exp."""
import torch


def rollout_reference(probs):
    """probs (layers, h, n, n) -> (layers, n - 1) float64: head mean, + identity, row-normalised, multiplied with the layer below (not with
    the running product), CLS row, scaled by the global maximum"""
    attn = torch.as_tensor(probs).double().mean(dim=1)
    attn = attn + torch.eye(attn.size(1), dtype=torch.float64)
    attn = attn / attn.sum(dim=-1, keepdim=True)
    res = torch.empty_like(attn)
    res[0] = attn[0]
    for i in range(1, attn.size(0)):
        res[i] = attn[i] @ attn[i - 1]
    res = res[:, 0, 1:]
    return res / res.max() if res.numel() else res


def rollout_rows(probs):
    """the unscaled closed-form rows: probs (layers, h, n, n) -> (c (layers, n), r (layers, n)) float64 with
    c_i[k] = (A_i[0,k] + [k == 0]) / 2,  r_0 = c_0,  r_i = (c_i A_{i-1} + c_i) / 2"""
    A = torch.as_tensor(probs).double().mean(dim=1)
    c = A[:, 0, :].clone()
    c[:, 0] += 1.0
    c = c / 2
    r = c.clone()
    for i in range(1, A.size(0)):
        r[i] = (c[i] @ A[i - 1] + c[i]) / 2
    return c, r


def rollout_closed_form(probs):
    """probs (layers, h, n, n) -> (layers, n - 1) float64 by the closed form (normaliser exactly 2)"""
    r = rollout_rows(probs)[1][:, 1:]
    return r / r.max() if r.numel() else r


def probs_from_qkv(qkv, lse, h, dh, scale):
    """one record: qkv (n, 3 h dh) (columns [q | k | v], head-major), lse (h, n) natural log -> P (h, n, n) float64 = exp(scale q k^T - lse)"""
    qkv, lse = torch.as_tensor(qkv).double(), torch.as_tensor(lse).double()
    n = qkv.shape[0]
    q = qkv[:, :h * dh].reshape(n, h, dh).permute(1, 0, 2)
    k = qkv[:, h * dh:2 * h * dh].reshape(n, h, dh).permute(1, 0, 2)
    return torch.exp(scale * (q @ k.transpose(1, 2)) - lse[:, :, None])


def lse_from_qkv(qkv, h, dh, scale):
    """one record: the exact log-sum-exp (h, n) float64 of its scores"""
    qkv = torch.as_tensor(qkv).double()
    n = qkv.shape[0]
    q = qkv[:, :h * dh].reshape(n, h, dh).permute(1, 0, 2)
    k = qkv[:, h * dh:2 * h * dh].reshape(n, h, dh).permute(1, 0, 2)
    return torch.logsumexp(scale * (q @ k.transpose(1, 2)), dim=-1)


def rollout_closed_form_qkv(qkvs, lses, h, dh, scale):
    """one record, per layer its qkv rows (n, 3 h dh) and lse (h, n) -> (layers, n - 1) float64"""
    return rollout_closed_form(torch.stack([probs_from_qkv(q, l, h, dh, scale) for q, l in zip(qkvs, lses)]))
