"""Worker of test_torch_autograd_through_regrid: gradients through ``Regridder.regrid`` on torch tensors that live on the GPU.
torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (initialised before the engine binds the device)

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adjoint_cases as ac  # noqa: E402
import xugrid_amd as xa  # noqa: E402
from xugrid_amd import meshgen  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_csr(rg):
    w = rg._ensure_host_weights()
    if hasattr(w, "indptr"):
        return np.asarray(w.data), np.asarray(w.indices).astype(np.int64), np.asarray(w.indptr).astype(np.int64), w.n, w.m
    indptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(w.row), minlength=w.n))]).astype(np.int64)
    return np.asarray(w.data), np.asarray(w.col).astype(np.int64), indptr, w.n, w.m


def main():
    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    sxy, sf = meshgen.triangle_mesh(1500, 61)
    txy, tf = meshgen.triangle_mesh(1250, 62, 30.0, 0.8)
    src_h = xa.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf)
    tgt_h = xa.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf)
    src_d = xa.Ugrid2d.from_device_arrays(t(sxy), t(sf))
    tgt_d = xa.Ugrid2d.from_device_arrays(t(txy), t(tf))
    rng = np.random.default_rng(8)
    S, T = sf.shape[0], tf.shape[0]
    data = rng.integers(-8, 9, size=(3, S)).astype(np.float64) / 4.0  # (exact in float32 as well)
    data[1, ::11] = np.nan
    c = rng.normal(size=(3, T))
    cases = ((xa.OverlapRegridder, {"method": "mean"}, "mean"), (xa.OverlapRegridder, {"method": "sum"}, "sum"),
             (xa.RelativeOverlapRegridder, {}, "first_order_conservative"), (xa.CentroidLocatorRegridder, {}, "select"),
             (xa.BarycentricInterpolator, {}, "mean"))
    for cls, kwargs, method in cases:
        # uploaded weights; for the flagship class also weights deferred to the first device call (device grids)
        for grids in ((src_h, tgt_h), (src_d, tgt_d))[: 2 if method == "mean" and cls is xa.OverlapRegridder else 1]:
            rg = cls(*grids, **kwargs)
            plain = rg.regrid(t(data))
            assert plain.grad_fn is None and not plain.requires_grad
            # nansum: the gradient is c where the output is a number, 0 where it is NaN (a NaN the locator copied included)
            g = np.where(np.isnan(plain.cpu().numpy()), 0.0, c)
            w_data, w_indices, w_indptr, n, m = host_csr(rg)
            ref = ac.adjoint_exact(method, w_data, w_indices, w_indptr, m, g, data)
            got64 = None
            for dtype in (torch.float64, torch.float32):
                leaf = t(data).to(dtype).requires_grad_()
                out = rg.regrid(leaf)
                assert out.grad_fn is not None and out.dtype == torch.float64
                assert np.array_equal(bits(out.detach().cpu().numpy()), bits(plain.cpu().numpy())), "the forward changed"
                torch.nansum(out * t(c)).backward()
                assert leaf.grad is not None and leaf.grad.dtype == dtype and tuple(leaf.grad.shape) == (3, S)
                got = leaf.grad.cpu().numpy()
                if dtype == torch.float64:
                    got64 = got
                    bad = ac.check_against_exact(got, ref)
                    assert not bad, (cls.__name__, method, bad[:5])
                    dev_adj = rg.regrid_adjoint(t(g), t(data))
                    assert isinstance(dev_adj, torch.Tensor) and np.array_equal(bits(dev_adj.cpu().numpy()), bits(got))
                else:  # the same float64 adjoint, cast to the leaf's dtype
                    assert got.dtype == np.float32 and np.array_equal(got, got64.astype(np.float32))
                if method != "select":
                    assert (got[np.isnan(data)] == 0).all()
            # without requires_grad, and under no_grad: today's path, today's bits, no grad_fn
            with torch.no_grad():
                leaf = t(data).requires_grad_()
                out = rg.regrid(leaf)
                assert out.grad_fn is None and not out.requires_grad
                assert np.array_equal(bits(out.cpu().numpy()), bits(plain.cpu().numpy()))
            # a leading batch dimension, and a graph that continues through the result
            leaf = t(np.stack([data, 2.0 * data])).requires_grad_()
            loss = torch.nansum(rg.regrid(leaf * 3.0) ** 2)
            loss.backward()
            # (d out^2 = 2 out: a NaN gradient on the rows the forward left NaN, which the adjoint ignores; the locator's rows
            # are live even where they copied a NaN, and plain IEEE applies there)
            assert tuple(leaf.grad.shape) == (2, 3, S) and (method == "select" or torch.isfinite(leaf.grad).all().item())
    # an unsupported reduction with a tensor that requires grad raises instead of cutting the graph
    rg = xa.OverlapRegridder(src_h, tgt_h, method="maximum")
    assert rg.regrid(t(data)).grad_fn is None
    try:
        rg.regrid(t(data).requires_grad_())
        raise SystemExit("maximum returned a result cut from the graph")
    except NotImplementedError as e:
        assert "maximum" in str(e)
    print("TORCH_ADJOINT_OK")


if __name__ == "__main__":
    main()
