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

Type 3 (``type3(plan, sources, targets, values)``, f_k = Σ_j c_j e^{sign i s_k·x_j}) is differentiable with respect to the values,
the sources and the targets (complex plans with ntransforms = 1).  Its adjoint is the type 3 of ``plan.adjoint()`` (sign −sign,
boxes swapped), u(x) = Σ_k G_k e^{−sign i s_k·x}:

    grad_s[k, d] = Re(conj(G_k) ∂f_k/∂s_d)        ∂f/∂s from exec_type3_grad in forward
    grad_c = u(x_j),  grad_x[j, d] = Re(c_j conj(∂_d u(x_j)))          one exec_type3_grad of the adjoint plan
"""
from __future__ import annotations

from typing import Sequence

import torch

from .plan import PlanNUFFT, exec_type1, exec_type2, exec_type2_grad, set_points
from .type3 import PlanNUFFT3, exec_type3, exec_type3_grad, set_points3


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


def _set3(plan: PlanNUFFT3, xs: tuple, ss: tuple):
    """set_points3 unless the plan already holds exactly these vectors."""
    cx, cs = plan._sources, plan._targets
    same = (cx is not None and cs is not None and len(cx) == len(xs) and len(cs) == len(ss)
            and all(a is b for a, b in zip(cx, xs)) and all(a is b for a, b in zip(cs, ss)))
    if not same:
        set_points3(plan, xs, ss)


def _adjoint3(plan: PlanNUFFT3) -> PlanNUFFT3:
    if plan._adjoint_plan is None:
        plan._adjoint_plan = plan.adjoint()
    return plan._adjoint_plan


class _Type3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, values, *coords):
        D = plan.ndim
        xs = tuple(x.detach().contiguous() for x in coords[:D])
        ss = tuple(s.detach().contiguous() for s in coords[D:])
        set_points3(plan, xs, ss)
        c = values.detach().contiguous()
        out = torch.empty(ss[0].numel(), dtype=plan.Z, device=c.device)
        grads = None
        if any(s.requires_grad for s in coords[D:]):
            grads = tuple(torch.empty_like(out) for _ in range(D))
            exec_type3_grad(out, grads, plan, c)
        else:
            exec_type3(out, plan, c)
        ctx.plan, ctx.xs, ctx.ss, ctx.grads = plan, xs, ss, grads
        ctx.save_for_backward(values, *coords)
        return out

    @staticmethod
    def backward(ctx, G):
        plan, xs, ss, grads = ctx.plan, ctx.xs, ctx.ss, ctx.grads
        values, *_ = ctx.saved_tensors
        D = plan.ndim
        G = G.resolve_conj().contiguous()
        need_c = ctx.needs_input_grad[1]
        need_x = any(ctx.needs_input_grad[2:2 + D])
        grad_c, grad_x, grad_s = None, [None] * D, [None] * D
        if need_c or need_x:
            adj = _adjoint3(plan)
            _set3(adj, ss, xs)
            u = torch.empty(xs[0].numel(), dtype=plan.Z, device=G.device)
            if need_x:
                du = tuple(torch.empty_like(u) for _ in range(D))
                exec_type3_grad(u, du, adj, G)
                c = values.detach()
                for d in range(D):
                    if ctx.needs_input_grad[2 + d]:
                        grad_x[d] = (c * du[d].conj()).real
            else:
                exec_type3(u, adj, G)
            grad_c = u if need_c else None
        Gc = G.conj()
        for d in range(D):
            if ctx.needs_input_grad[2 + D + d]:
                grad_s[d] = (Gc * grads[d]).real
        return (None, grad_c, *grad_x, *grad_s)


def type3(plan: PlanNUFFT3, sources, targets, values: torch.Tensor) -> torch.Tensor:
    """Differentiable type 3: returns a new vector of Nk values (sets the plan's points).  ``sources`` / ``targets``: tuples of D
    real vectors (or (N, D) tensors) inside the plan's boxes; points outside them give undefined results, as in exec_type3.
    The backward pass for the values or the sources runs on ``plan.adjoint()``, created on first use and cached on ``plan``: it
    holds a second set of grids of the same size, so it doubles the plan's grid memory."""
    if plan.ntransforms != 1:
        raise ValueError("autograd supports plans with ntransforms = 1")
    D = plan.ndim

    def vecs(p, what):
        if isinstance(p, torch.Tensor):
            p = (p,) if p.dim() == 1 else tuple(p[:, d] for d in range(p.shape[1]))
        p = tuple(p)
        if len(p) != D:
            raise ValueError(f"expected {D} {what} coordinate vectors")
        return p

    return _Type3.apply(plan, values, *vecs(sources, "source"), *vecs(targets, "target"))
