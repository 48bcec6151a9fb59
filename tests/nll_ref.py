"""fp64 reference of the pixel-to-segment NLL (include/spml_hip.h, A9/A10), written from the header's formula in plain
torch operations; gradients by autograd.  CPU only: the yardstick of tests/test_nll_branches_gpu.py.

  sim       = exp(kappa * E Pr^T)                                  [P, M]
  same      = px_code == pr_code  (LABEL)  |  (px_code & pr_code) != 0  (TAGSET)
  own_sim   = sim[p, own[p]]
  pos       = sum_same sim - own_sim
  fallback  = PLAIN or pos <= 0:  num = own_sim, else num = pos
  den       = sum_{not same} sim + num
  nll       = -log(num / den)
  stats     = (num, den, own_sim, fallback)
"""
import torch

TAGSET, PLAIN, CODE32 = 1, 2, 4


class NllRef:
  """nll [P], stats [P, 4], pos [P] (sum_same - own_sim, before the fallback), own_same [P] (the own prototype is in
  the pixel's positive set), d_emb [P, D], d_protos [M, D] for the upstream gradient given -- all fp64."""


def positive_mask(px_code, pr_code, mode):
  if mode & TAGSET:
    return (px_code.view(-1, 1) & pr_code.view(1, -1)) != 0
  return px_code.view(-1, 1) == pr_code.view(1, -1)


def forward(emb, own, px_code, protos, pr_code, kappa, mode, dtype=torch.float64):
  """-> nll, stats, pos, own_same in `dtype` (differentiable with respect to emb / protos)."""
  sim = ((emb.to(dtype) @ protos.to(dtype).t()) * kappa).exp()
  same = positive_mask(px_code, pr_code, mode)
  own_sim = sim.gather(1, own.view(-1, 1)).view(-1)
  pos = (sim * same.to(dtype)).sum(1) - own_sim
  fallback = torch.ones_like(pos, dtype=torch.bool) if mode & PLAIN else ~(pos > 0)
  num = torch.where(fallback, own_sim, pos)
  den = (sim * (~same).to(dtype)).sum(1) + num
  nll = -(num / den).log()
  stats = torch.stack([num, den, own_sim, fallback.to(dtype)], 1)
  own_same = same.gather(1, own.view(-1, 1)).view(-1)
  return nll, stats, pos, own_same


def evaluate(emb, own, px_code, protos, pr_code, kappa, mode, d_nll=None, dtype=torch.float64):
  """The reference of one call.  d_nll [P]: upstream gradient (None: forward only)."""
  r = NllRef()
  e = emb.detach().to(dtype).clone().requires_grad_(d_nll is not None)
  pr = protos.detach().to(dtype).clone().requires_grad_(d_nll is not None)
  nll, stats, pos, own_same = forward(e, own, px_code, pr, pr_code, kappa, mode, dtype)
  r.nll, r.stats, r.pos, r.own_same = nll.detach(), stats.detach(), pos.detach(), own_same
  r.d_emb = r.d_protos = None
  if d_nll is not None:
    (nll * d_nll.to(dtype)).sum().backward()
    r.d_emb, r.d_protos = e.grad, pr.grad
  return r


def d_protos_rows(d_protos, m_grad):
  """What a backward call with this m_grad must leave in a zeroed d_protos: (lo, hi, want) -- rows [0, lo) equal
  want, rows [hi, M) are exactly zero, a row in [lo, hi) is either zero or want's (whole 32-prototype tiles)."""
  m = d_protos.shape[0]
  mg = m if m_grad < 0 or m_grad > m else m_grad
  return mg, min(m, (mg + 31) // 32 * 32), d_protos
