"""A float64 restatement of torch.optim.Adam (no amsgrad, L2 weight decay ``g + wd * p``), and the error yardstick the GPU
tests measure the fused kernels with.  Plain torch, no project code.

The yardstick.  One step from a float32 state is compared with the float64 restatement from that same state; the error of each
result is expressed in units of 2^-24 (the unit round-off of float32) times the magnitude of the OPERANDS of the update that
produced it -- not of the result, which cancels (``lerp`` for m, ``p - dp`` for p) and would turn rounding into thousands of "ulps":

    m:  |m0| + g^            v:  v0 + g^ ** 2            p:  |p0| + dp^

    g^  = |g| + wd * |p0|                                            (= |g'|, g' = g + wd * p0, unless the two cancel)
    dp^ = lr / bc1 * (b1 |m0| + (1 - b1) g^) / (sqrt(v') / sqrt(bc2) + eps) * (b2 v0 + (1 - b2) g^ ** 2) / v'
                                                                     (= |dp| unless m0 and g', or g and wd * p0, cancel)

Why the operands of g' and of dp, too.  A first measurement scaled by |g'| and by |dp| = |p' - p0|.  Both are results: with wd > 0
an element whose g is close to -wd * p0 has a g' far below its operands, and an element whose b1 * m0 is close to -(1 - b1) * g'
has an m' -- hence a dp -- far below its operands.  torch's own float32 Adam then showed 1100 units on m, 220 on v and 560 on p
(2.5 million elements; without weight decay still 17 on p), figures that only measure how close the nearest cancellation among
the random elements happened to come and grow with the element count.  Scaled by the operands the figures are flat in the element
count; where nothing cancels (same signs; for g^ also wd = 0) every scale above equals the plain |m0| + |g'|, v0 + g'^2, |p0| + |dp|.

Measured (tests/test_adam_ref_host.py::test_float32_torch_adam_stays_within_the_recorded_units: torch's own float32 CPU Adam, 2^16
elements per case, p in 1e-4 .. 1e2 and g in 1e-8 .. 1e3 log-uniform with random signs, m and v of the same range, 19 combinations
of wd in {0, 1e-2}, eps in {1e-8, 1e-4}, three beta pairs and steps 1 .. 10^6, each at lr 1e-3 and 1e-1), worst case over all:

    m: 1.36 units      v: 2.16 units      p: 6.29 units

TORCH_F32_UNITS records them rounded up, the host test asserts torch's float32 Adam stays within them, and a fused GPU kernel is
held to GPU_FACTOR = 4 times that: it may contract ``a * b + c`` into one fma, keeps ``1 / sqrt(bc2)`` and ``lr / bc1`` as rounded
float32 factors, takes ``1 - beta`` from the float32 beta and reorders where torch does not; 4 x still catches a wrong formula (a
missing bias correction, a step count off by one, decoupled weight decay) by orders of magnitude
(test_units_see_a_wrong_formula_from_far_away)."""
import torch

U = 2.0 ** -24
TORCH_F32_UNITS = {"m": 1.5, "v": 2.5, "p": 7.0}          # measured: see the module docstring
GPU_FACTOR = 4.0


def adam_step64(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """One Adam step in float64 from float32 (or any) ``p, g, m, v``; ``step`` >= 1 is the number of THIS step.  Returns float64
    ``p', m', v'``."""
    p, g, m, v = (t.detach().double() for t in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    gp = g + float(wd) * p
    m1 = b1 * m + (1.0 - b1) * gp
    v1 = b2 * v + (1.0 - b2) * gp * gp
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    p1 = p - (float(lr) / bc1) * m1 / (v1.sqrt() / bc2 ** 0.5 + float(eps))
    return p1, m1, v1


def scales(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """Operand magnitudes (float64) the errors of ``m', v', p'`` are measured against (module docstring)."""
    p, g, m, v = (t.detach().double() for t in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    gp = g + float(wd) * p
    gh = g.abs() + float(wd) * p.abs()                       # the operands of g'; equal to |g'| unless the two cancel
    m_ops = b1 * m.abs() + (1.0 - b1) * gh                   # the operands of m'; equal to |m'| unless m0 and g' cancel
    v_ops = b2 * v + (1.0 - b2) * gh * gh                    # the operands of v'; equal to v' unless g and wd * p cancel
    v1 = b2 * v + (1.0 - b2) * gp * gp
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    dp_ops = (float(lr) / bc1) * m_ops / (v1.sqrt() / bc2 ** 0.5 + float(eps))
    dp_ops = torch.where(v1 > 0, dp_ops * (v_ops / v1.clamp_min(1e-300)), dp_ops)
    return {"m": m.abs() + gh, "v": v + gh * gh, "p": p.abs() + dp_ops}


UNDERFLOW = 2.0 ** -126       # the smallest normal float32: below it a result is a multiple of 2^-149, or flushed to zero, whatever the formula


def units(got, want, scale):
    """|got - want| in units of 2^-24 * scale, element-wise (float64); 0 where the error is 0 or below float32's normal range (a
    gradient of 1e-25 has a square no float32 holds: that is the format, not the update rule)."""
    err = ((got.detach().double() - want).abs() - UNDERFLOW).clamp_min(0.0)
    return torch.where(err == 0, torch.zeros_like(err), err / (U * scale))


def worst_units(got_pmv, state, step, lr, betas, eps, wd):
    """{"p": .., "m": .., "v": ..}: the largest error, in units, of one step ``got_pmv`` = (p', m', v') taken from ``state`` =
    (p, g, m, v); non-finite results count as infinite."""
    p, g, m, v = state
    p1, m1, v1 = adam_step64(p, g, m, v, step, lr, betas, eps, wd)
    sc = scales(p, g, m, v, step, lr, betas, eps, wd)
    out = {}
    for name, got, want in (("p", got_pmv[0], p1), ("m", got_pmv[1], m1), ("v", got_pmv[2], v1)):
        un = units(got, want, sc[name])
        out[name] = float(torch.nan_to_num(un, nan=float("inf")).max()) if un.numel() else 0.0
    return out


def gpu_bound(name):
    return GPU_FACTOR * TORCH_F32_UNITS[name]
