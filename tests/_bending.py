"""float64 torch restatement of the bending energy (HessianOperator: GradientOperator applied twice), written out as the closed
form and NOT through the package's operators.  CPU or GPU tensors, any float dtype in, float64 out.

Per chain and component f, with w(q) = 2 for q = n - 2 and 1 otherwise (the replicated last first difference counts twice):

  pure terms   for each axis a with n_a >= 3: (f[i+2] - 2 f[i+1] + f[i])^2 over i <= n_a - 3 and every position of the other two
               axes, weight 1 (the two replicated planes of a second difference along its own axis are exactly 0);
  mixed terms  for each pair a < b: TWICE the sum of w_a(i) w_b(j) (f[i+1,j+1] - f[i,j+1] - f[i+1,j] + f[i,j])^2 over
               i <= n_a - 2, j <= n_b - 2 and every position of the third axis.

`energy(v)`    y per chain, (C,) float64.
`grad(v)`      dy/dv by autograd of the closed form: 2 H^T W H v.
`grad_abs(v)`  the same adjoint with every coefficient of H and H^T and every value replaced by its absolute value:
               2 |H|^T W |H| |v|, the a-priori magnitude of what rounding can do to one output (no tap of H^T W H collects
               contributions of both signs, so this is also |2 H^T W H| |v|).
"""
import torch

_AXES = (2, 3, 4)


def _w(n, like):
    w = torch.ones(n - 1, dtype=torch.float64, device=like.device)
    w[n - 2] = 2.0
    return w


def _shape_for(w, axis):
    s = [1] * 5
    s[axis] = w.numel()
    return w.reshape(s)


def _quadratic(f, sign):
    """sum of the weighted squared stencil responses per chain; sign = -1: the operator H, sign = +1: |H| (every coefficient
    replaced by its absolute value)"""
    y = torch.zeros(f.shape[0], dtype=torch.float64, device=f.device)
    for a in _AXES:
        n = f.shape[a]
        if n >= 3:
            s = f.narrow(a, 2, n - 2) + sign * 2.0 * f.narrow(a, 1, n - 2) + f.narrow(a, 0, n - 2)
            y = y + (s ** 2).sum(dim=(1, 2, 3, 4))
    for ia, a in enumerate(_AXES):
        for b in _AXES[ia + 1:]:
            na, nb = f.shape[a], f.shape[b]
            hi, lo = f.narrow(a, 1, na - 1), f.narrow(a, 0, na - 1)
            d = (hi.narrow(b, 1, nb - 1) + sign * lo.narrow(b, 1, nb - 1)) + sign * (hi.narrow(b, 0, nb - 1) + sign * lo.narrow(b, 0, nb - 1))
            w = _shape_for(_w(na, f), a) * _shape_for(_w(nb, f), b)
            y = y + 2.0 * (w * d ** 2).sum(dim=(1, 2, 3, 4))
    return y


def energy(v):
    return _quadratic(v.detach().to(torch.float64), -1.0)


def _grad_of(f, sign):
    with torch.enable_grad():
        f = f.clone().requires_grad_(True)
        g, = torch.autograd.grad(_quadratic(f, sign).sum(), f)
    return g


def grad(v):
    return _grad_of(v.detach().to(torch.float64), -1.0)


def grad_abs(v):
    return _grad_of(v.detach().to(torch.float64).abs(), 1.0)
