"""The one place in tests/ that starts ranks: several processes that share one GPU (or the CPU) and are joined over gloo, or
one process on RCCL.  A test calls ``launch(worker, world, *args, limit=seconds)``; the worker is

    def _worker_x(rank, world, rendezvous, *args):
        with ranks(rank, world, rendezvous) as dist:
            ...

No pytest-level timeout exists, so ``launch`` is where a hung rank is ended: every launch has a time limit, no collective
waits longer than that limit, and whatever is still alive when ``launch`` returns or raises is killed and joined.  The ranks
meet over a file in a temporary directory, not over a TCP port: no port is probed, so none can be taken between the probe and
the bind.  Nothing here is product code.
"""
import contextlib
import datetime
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WORLD = 15                     # the pytest process holds the GPU too, and the GPU boxes allow 16 processes with it open
_LIMIT_ENV = "MAKANI_AMD_TEST_RANKS_LIMIT"      # launch -> join_group: the launch limit, the default collective timeout


def share_gpu(rank, world, ncu=256):
    """Round 5 gave the ranks that share ONE GPU in a test disjoint compute units (``HSA_CU_MASK``) because kernels of different
    processes on one compute unit disturbed each other's results.  Round 6 found the cause — packed-fp32 instructions that read a
    VGPR src1 through op_sel are unreliable on gfx950 while certain matrix-core kernels share the compute unit
    (docs/LAB_NOTEBOOK.md 6.1, tools/pk_hazard_probe.py) — and removed those instruction forms from every kernel
    (tools/pk_opsel_scan.py, tests/test_packed_forms.py).  The tests therefore run WITHOUT the mask: N ranks on one GPU share
    all compute units, which is the stronger check.  ``MAKANI_AMD_TEST_CU_MASK=1`` brings the mask back (must be in the
    environment before the process's first GPU call)."""
    if os.environ.get("MAKANI_AMD_TEST_CU_MASK", "0") != "1":
        return
    per = max(1, ncu // max(1, world))
    os.environ["HSA_CU_MASK"] = f"0:{rank * per}-{(rank + 1) * per - 1}"


def launch(worker, world, *args, limit):
    """``worker(rank, world, rendezvous, *args)`` in ``world`` processes, ended after ``limit`` seconds: a schedule bug between
    ranks is a hang, and a hung GPU box is worse than a red test.  A failing rank's traceback propagates; nothing is retried."""
    if world > MAX_WORLD:
        raise ValueError(f"{worker.__name__}: {world} ranks, at most {MAX_WORLD} may be started")
    import torch.multiprocessing as mp
    t0 = time.monotonic()
    ctx = None
    with tempfile.TemporaryDirectory() as tmp:
        os.environ[_LIMIT_ENV] = repr(float(limit))          # the children inherit it
        try:
            ctx = mp.spawn(worker, args=(world, os.path.join(tmp, "rendezvous"), *args), nprocs=world, join=False)
            while not ctx.join(timeout=min(5.0, max(0.0, limit - (time.monotonic() - t0)))):
                if time.monotonic() - t0 >= limit:
                    raise TimeoutError(f"{worker.__name__}: {world} ranks did not finish within {limit} s")
        finally:
            del os.environ[_LIMIT_ENV]
            procs = ctx.processes if ctx is not None else []
            for p in procs:
                if p.is_alive():
                    p.kill()
            for p in procs:
                p.join()


def join_group(rank, world, rendezvous, backend="gloo", timeout=None, device=None):
    """the prologue of a worker: the repository and tests/ importable, the process group of the launch joined over its
    rendezvous file.  ``timeout`` (seconds) of the collectives defaults to the launch limit."""
    import torch
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
    kw = {}
    if backend == "nccl":
        torch.cuda.set_device(device)
        kw["device_id"] = device
    else:
        share_gpu(rank, world)              # before the first GPU call
    seconds = float(os.environ[_LIMIT_ENV]) if timeout is None else timeout
    dist.init_process_group(backend, init_method="file://" + rendezvous, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=seconds), **kw)
    return dist


@contextlib.contextmanager
def ranks(rank, world, rendezvous, backend="gloo", timeout=None, device=None):
    """``join_group`` and the epilogue of a worker: a barrier on the clean path, the process group destroyed on every path"""
    dist = join_group(rank, world, rendezvous, backend, timeout, device)
    try:
        yield dist
        dist.barrier()
    finally:
        dist.destroy_process_group()


def hw_groups(rank, h, w):
    """(ih, iw, hg, wg) of rank = ih * w + iw in an h x w grid: the column groups, then the row groups, created in the same
    order on every rank; hg joins the h ranks of this rank's column, wg the w ranks of its row"""
    import torch.distributed as dist
    ih, iw = rank // w, rank % w
    hg = wg = None
    for j in range(w):
        g = dist.new_group([i * w + j for i in range(h)])
        if j == iw:
            hg = g
    for i in range(h):
        g = dist.new_group([i * w + j for j in range(w)])
        if i == ih:
            wg = g
    return ih, iw, hg, wg


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
