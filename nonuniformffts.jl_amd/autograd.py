"""torch.autograd through type 1 and type 2, with respect to the values / the spectrum and the points.

    f = type1(plan, points, values)    f_k = Σ_j c_j e^{−i k·x_j}     (plan.shape, complex)
    v = type2(plan, points, uhat)      v_j = Σ_k û_k e^{+i k·x_j}     (Np, complex)

``points`` is a tuple of D real vectors of the plan's precision (any of them may require grad).  Complex plans with
ntransforms = 1 only: the half-spectrum adjoint of a real plan is not a plain type 2.

The computed type 1 and type 2 of one plan are exact adjoints of each other (the type-1 normalisation prod(2π/Ñ_d) equals the
interpolation prefactor), so the vector-Jacobian products — in torch's conjugate-Wirtinger convention, G the upstream
gradient — are transforms of the same plan:

    type 1:  grad_c = type2(G),  grad_x[j, d] = Re(c_j conj(∂_d type2(G)(x_j)))          one exec_type2_grad
    type 2:  grad_û = type1(g),  grad_x[j, d] = Re(conj(g_j) ∂_d v(x_j))                 ∂_d v from exec_type2_grad in forward

Each call of ``type1`` / ``type2`` sets the plan's points; ``backward`` sets them again only if the plan holds other points by
then.
"""
from __future__ import annotations

from typing import Sequence

import torch

from .plan import PlanNUFFT, exec_type1, exec_type2, exec_type2_grad, set_points


def _check_plan(plan: PlanNUFFT):
    if not plan.is_complex:
        raise ValueError("autograd needs a complex plan: the adjoint of a real plan's half spectrum is not a plain type 2")
    if plan.ntransforms != 1:
        raise ValueError("autograd supports plans with ntransforms = 1")


def _points_tuple(plan: PlanNUFFT, points) -> tuple:
    if isinstance(points, torch.Tensor):
        points = (points,) if points.dim() == 1 else tuple(points[:, d] for d in range(points.shape[1]))
    points = tuple(points)
    if len(points) != plan.ndim:
        raise ValueError(f"expected {plan.ndim} coordinate vectors")
    return points


def _set(plan: PlanNUFFT, points: Sequence[torch.Tensor]) -> tuple:
    held = tuple(x.detach().contiguous() for x in points)
    set_points(plan, held)
    return held


def _ensure(plan: PlanNUFFT, held: tuple):
    cur = plan.points
    if cur is None or len(cur) != len(held) or any(a is not b for a, b in zip(cur, held)):
        set_points(plan, held)


def _empty_np(plan: PlanNUFFT, n: int, like: torch.Tensor):
    return torch.empty(n, dtype=plan.Z, device=like.device)


class _Type1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, values, *points):
        held = _set(plan, points)
        out = torch.empty(plan.shape, dtype=plan.Z, device=values.device)
        exec_type1(out, plan, values.detach().contiguous())
        ctx.plan, ctx.held = plan, held
        ctx.save_for_backward(values, *points)
        return out

    @staticmethod
    def backward(ctx, G):
        plan, held = ctx.plan, ctx.held
        values, *points = ctx.saved_tensors
        _ensure(plan, held)
        G = G.resolve_conj().contiguous()
        n = values.numel()
        need_c = ctx.needs_input_grad[1]
        need_x = any(ctx.needs_input_grad[2:])
        grad_c, grad_x = None, [None] * len(points)
        if need_x:
            grads = tuple(_empty_np(plan, n, G) for _ in points)
            vp = _empty_np(plan, n, G) if need_c else None
            exec_type2_grad(grads, plan, G, vp=vp)
            grad_c = vp
            c = values.detach()
            for d, gd in enumerate(grads):
                if ctx.needs_input_grad[2 + d]:
                    grad_x[d] = (c * gd.conj()).real
        elif need_c:
            grad_c = _empty_np(plan, n, G)
            exec_type2(grad_c, plan, G)
        return (None, grad_c, *grad_x)


class _Type2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, uhat, *points):
        held = _set(plan, points)
        n = held[0].numel()
        u = uhat.detach().contiguous()
        out = _empty_np(plan, n, u)
        need_x = any(x.requires_grad for x in points)
        grads = None
        if need_x:
            grads = tuple(_empty_np(plan, n, u) for _ in points)
            exec_type2_grad(grads, plan, u, vp=out)
        else:
            exec_type2(out, plan, u)
        ctx.plan, ctx.held, ctx.grads = plan, held, grads
        ctx.save_for_backward(uhat, *points)
        return out

    @staticmethod
    def backward(ctx, g):
        plan, held, grads = ctx.plan, ctx.held, ctx.grads
        ctx.saved_tensors        # (raises if the spectrum or the points were modified in place since forward)
        g = g.resolve_conj().contiguous()
        grad_u, grad_x = None, [None] * len(held)
        if ctx.needs_input_grad[1]:
            _ensure(plan, held)
            grad_u = torch.empty(plan.shape, dtype=plan.Z, device=g.device)
            exec_type1(grad_u, plan, g)
        gc = g.conj()
        for d in range(len(held)):
            if ctx.needs_input_grad[2 + d]:
                grad_x[d] = (gc * grads[d]).real
        return (None, grad_u, *grad_x)


def type1(plan: PlanNUFFT, points, values: torch.Tensor) -> torch.Tensor:
    """Differentiable type 1: returns a new array of shape plan.shape (sets the plan's points)."""
    _check_plan(plan)
    return _Type1.apply(plan, values, *_points_tuple(plan, points))


def type2(plan: PlanNUFFT, points, uhat: torch.Tensor) -> torch.Tensor:
    """Differentiable type 2: returns a new vector of Np values (sets the plan's points)."""
    _check_plan(plan)
    return _Type2.apply(plan, uhat, *_points_tuple(plan, points))
