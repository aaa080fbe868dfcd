"""What the ensemble losses (``losses.py``) and the ensemble metrics (``metrics.py``) share: the input checks, the limit on the
ensemble size, and the ensemble-parallel path — every rank of the "ensemble" group trades its members for ALL members on a
share of the points, scores that share, and the shares are summed."""
import torch

MAX_ENSEMBLE = 32          # members of a grid point live in registers (csrc/crps.hip)


def ensemble_size_check(E, what):
    """``what`` names the kernel family ("CRPS", "energy-score", "likelihood", "MMD", "metric")"""
    if E > MAX_ENSEMBLE:
        raise NotImplementedError(f"ensemble size {E}: the HIP {what} kernels are built for at most {MAX_ENSEMBLE} members per point")


def check_forecast_dims(forecasts):
    if forecasts.dim() != 5:
        raise ValueError(f"Error, forecasts tensor expected to have 5 dimensions but found {forecasts.dim()}.")


def check_weight_dims(weights, observations, found=True):
    """``found``: the message counts the dimensions (the reference's likelihood and spectral CRPS losses do not)"""
    if weights is not None and weights.dim() != observations.dim():
        if not found:
            raise ValueError("the weights have to have the same number of dimensions as observations")
        raise ValueError(f"the weights have to have the same number of dimensions (found {weights.dim()}) as "
                         f"observations (found {observations.dim()}).")


class EnsembleTransposeFn(torch.autograd.Function):
    """``distributed_transpose(forecasts, (-1, 0), ensemble_shapes, "ensemble")`` of ``crps_loss.py:362-366,566-570``: every
    rank of the ensemble group holds E_loc members on all N points and ends up with ALL members on its share of the points
    (``compute_split_shapes(N, n)``).  x (B, E_loc, C, N) -> (B, E_loc * n, C, N_loc); backward is the reverse exchange."""

    @staticmethod
    def forward(ctx, x, group):
        import torch.distributed as dist
        from . import distributed as thd
        n, me = dist.get_world_size(group), dist.get_rank(group)
        B, El, Cc, N = x.shape
        sizes = thd.compute_split_shapes(N, n)
        off = [0]
        for v in sizes:
            off.append(off[-1] + v)
        send = [x[..., off[r]:off[r + 1]].contiguous() for r in range(n)]
        recv = [torch.empty((B, El, Cc, sizes[me]), dtype=x.dtype, device=x.device) for _ in range(n)]
        thd._exchange(recv, send, group)
        ctx.meta = (group, n, me, sizes, off, N)
        return torch.cat(recv, dim=1)

    @staticmethod
    def backward(ctx, g):
        from . import distributed as thd
        group, n, me, sizes, off, N = ctx.meta
        B, E, Cc, Nl = g.shape
        El = E // n
        send = [g[:, r * El:(r + 1) * El].contiguous() for r in range(n)]
        recv = [torch.empty((B, El, Cc, sizes[r]), dtype=g.dtype, device=g.device) for r in range(n)]
        thd._exchange(recv, send, group)
        return torch.cat(recv, dim=3), None


def ensemble_split(forecasts, obs, q, wgt):
    """the ensemble-parallel path of the CRPS losses: (forecasts with ALL members on this rank's share of the points, that
    share of the observations / quadrature weights / spatial weights, the group).  forecasts (B, E_loc, C, N) etc."""
    import torch.distributed as dist
    from . import comm as _comm
    from . import distributed as thd
    group = _comm.get_group("ensemble")
    n, me = dist.get_world_size(group), dist.get_rank(group)
    N = forecasts.shape[-1]
    sizes = thd.compute_split_shapes(N, n)
    a = sum(sizes[:me])
    b = a + sizes[me]
    f = EnsembleTransposeFn.apply(forecasts, group)
    return f, obs[..., a:b].contiguous(), q[..., a:b].contiguous(), (wgt[..., a:b].contiguous() if wgt is not None else None), group


def flatten_and_split(forecasts, observations, q, weights, ensemble_distributed):
    """forecasts (B, E, C, H, W), observations (B, C, H, W), q (H * W), weights broadcastable to the observations or None ->
    f (B, E, C, N), o (B, C, N), q (N), w (B, C, N) | None and the ensemble group: with ``ensemble_distributed`` N is this
    rank's share of the H * W points and E counts the members of the whole group, else the group is None."""
    B, E, Cc, H, W = forecasts.shape
    f = forecasts.reshape(B, E, Cc, H * W)
    o = observations.reshape(B, Cc, H * W)
    w = weights.expand(B, Cc, H, W).reshape(B, Cc, H * W) if weights is not None else None
    if not ensemble_distributed:
        return f, o, q, w, None
    return ensemble_split(f, o, q, w)


class ReduceFromGroupFn(torch.autograd.Function):
    """``reduce_from_parallel_region``: SUM all-reduce forward, identity backward"""

    @staticmethod
    def forward(ctx, x, group):
        from . import ops
        y = x.clone()
        ops._all_reduce_sum(y, group)
        return y

    @staticmethod
    def backward(ctx, g):
        return g, None


def ensemble_active(flag) -> bool:
    """``ensemble_distributed`` is honoured when the process-group tree names a split "ensemble" group.  The tree may not have
    been looked at yet (a loss constructed before any makani_amd network under makani's own driver): adopt makani's tree first;
    a set flag without such a group in a multi-rank job is reported — each rank would otherwise silently score its local
    members only."""
    if not flag:
        return False
    from . import comm as _comm
    _comm.autodetect()
    active = _comm.is_distributed("ensemble") and _comm.get_size("ensemble") > 1
    if not active and _comm.get_world_size() > 1:
        import warnings
        warnings.warn("ensemble_distributed=True, but the process-group tree has no split 'ensemble' group: the loss scores the "
                      "members of this rank only (makani_amd.comm.init(h, w, ensemble=n) or makani's own tree provides the group)")
    return active
