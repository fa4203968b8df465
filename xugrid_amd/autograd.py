"""
``regrid`` inside a torch autograd graph.

``Regridder.regrid(tensor)`` hands device pointers to the engine, which torch cannot see through.  For a tensor that
requires grad the call goes through the Function below instead: the forward is the same device apply
(``BaseRegridder._regrid_device``), the backward is ``BaseRegridder.regrid_adjoint`` -- the transposed-weights apply of
xr_adjoint.hip with the forward input's NaN pattern.  Served: the reductions that are linear in the data (mean, sum,
first_order_conservative / conductance, the centroid locator, the barycentric interpolator); any other method raises
NotImplementedError before anything runs.  Double backward is not offered (``once_differentiable``).

torch is imported lazily, as everywhere in this package.
"""
from . import engine

_function = None


def grad_enabled() -> bool:
    import torch

    return torch.is_grad_enabled()


def _regrid_function():
    global _function
    if _function is None:
        import torch
        from torch.autograd.function import once_differentiable

        class Regrid(torch.autograd.Function):
            @staticmethod
            def forward(ctx, data, regridder):
                detached = data.detach()
                ctx.regridder = regridder
                ctx.save_for_backward(detached)  # (its NaN pattern decides the mean's denominators)
                return regridder._regrid_device(detached, engine.device_array_info(detached))

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_out):
                (data,) = ctx.saved_tensors
                grad = grad_out.to(torch.float64).contiguous()
                # (regrid_adjoint drains torch's current stream before the engine reads `grad`, as sync_producer does for
                # the forward input, and returns with the result complete)
                out = ctx.regridder.regrid_adjoint(grad, data)
                return out.to(data.dtype), None

        _function = Regrid
    return _function


def regrid(regridder, data):
    """``regridder.regrid(data)`` for a GPU tensor that requires grad: the result carries a ``grad_fn``."""
    regridder._adjoint_method()  # NotImplementedError for a reduction without an adjoint
    info = engine.device_array_info(data)  # (raises for a tensor that is not contiguous, as the plain path does)
    if info[2].name not in ("float64", "float32"):
        raise TypeError(f"device data must be float64 or float32, received {info[2]}")
    return _regrid_function().apply(data, regridder)
