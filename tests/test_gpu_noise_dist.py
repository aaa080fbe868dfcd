"""The noise processes on a sphere split over h x w ranks (makani_amd/noise.py over mk_noise_update_shard and
DistributedInverseRealSHT), several processes sharing cuda:0 over gloo in the pattern of tests/test_gpu_distributed.py.

The counter of an element is its GLOBAL index, so ranks that share a seed hold exactly the slices of the serial state: the shards
are compared with the serial module's state by torch.equal, the synthesised fields within the relative 1e-5 of
test_distributed_sht_ragged_config3_splits_on_the_hip_backend (the reference's own tolerance for its distributed layers).
Grid 37 x 72, lmax = mmax = 37: over two ranks l, m and the latitudes split [19, 18] (ragged, and m0 = 19 is odd: the second w
rank's floats start in the middle of a Philox group), the longitudes [36, 36]."""
import pytest
import torch

from _ranks import launch, ranks, rel

pytestmark = pytest.mark.gpu
IMG, B, C = (37, 72), 2, 3
TOL = 1e-5


def _build(ma):
    """the modules under test, from fixed seeds: serial before the groups exist, split afterwards"""
    kT, lambd = [1e-3 * (c + 1) for c in range(C)], [0.5 + 0.5 * c for c in range(C)]
    return {"diffusion T=1": ma.DiffusionNoiseS2(IMG, B, C, num_time_steps=1, kT=kT, lambd=lambd, seed=11),
            "diffusion T=2": ma.DiffusionNoiseS2(IMG, B, C, num_time_steps=2, kT=kT, lambd=lambd, seed=12, reflect=True),
            "white": ma.IsotropicGaussianRandomFieldS2(IMG, B, C, num_time_steps=2, alpha=1.0, seed=13),
            "white learnable": ma.IsotropicGaussianRandomFieldS2(IMG, B, C, alpha=0.5, seed=14, learnable=True),
            "dummy": ma.DummyNoiseS2(IMG, B, C, num_time_steps=2, mode="constant_random", seed=15)}


def _run(m):
    """replace, then two further updates: the states, and the field after each stage"""
    out = []
    m.update(replace_state=True)
    out.append((m.get_tensor_state(), m().detach().clone()))
    m.update()
    m.update()
    out.append((m.get_tensor_state(), m().detach().clone()))
    return out


def _worker(rank, world, rendezvous, h, w):
    with ranks(rank, world, rendezvous) as dist:
        import makani_amd as ma
        import makani_amd.comm as mcomm
        import makani_amd.distributed as thd
        dev = torch.device("cuda:0")
        was = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.manual_seed(3)
        G = torch.randn(B, 1, C, *IMG, device=dev)

        # ---- the serial modules, from the same seeds, before the groups are initialised
        serial = {k: m.to(dev) for k, m in _build(ma).items()}
        assert not any(m.spatial_parallel for m in serial.values())
        want = {k: _run(m) for k, m in serial.items() if k != "white learnable"}
        sl = serial["white learnable"]
        sl.update()
        (want_grad,) = torch.autograd.grad((sl() * G).sum(), sl.sigma_l)

        # ---- the same modules on the split sphere
        _, ih, iw = mcomm.init(h, w)
        assert thd.ensure_initialized()
        split = {k: m.to(dev) for k, m in _build(ma).items()}
        m0 = split["diffusion T=1"]
        assert m0.spatial_parallel and isinstance(m0.isht, thd.DistributedInverseRealSHT) and (m0.lmax, m0.mmax) == (37, 37)
        two = [19, 18]
        assert m0.isht.l_shapes == (two if h == 2 else [37]) and m0.isht.lat_shapes == (two if h == 2 else [37])
        assert m0.isht.m_shapes == (two if w == 2 else [37]) and m0.isht.lon_shapes == ([36, 36] if w == 2 else [72])
        l0, ll, mo, ml = m0.l_off, m0.lmax_local, m0.m_off, m0.mmax_local
        la0, hl, lo0, wl = m0.lat_off, m0.nlat_local, m0.lon_off, m0.nlon_local
        assert (l0, ll) == ((19 * ih, two[ih]) if h == 2 else (0, 37)) and (mo, ml) == ((19 * iw, two[iw]) if w == 2 else (0, 37))
        assert (la0, hl) == (l0, ll) and (lo0, wl) == ((36 * iw, 36) if w == 2 else (0, 72))
        spec = (Ellipsis, slice(l0, l0 + ll), slice(mo, mo + ml), slice(None))
        grid = (Ellipsis, slice(la0, la0 + hl), slice(lo0, lo0 + wl))

        # 6. the spectral processes: sigma_l shards, states bit for bit, fields at the distributed transform's tolerance
        for k in ("diffusion T=1", "diffusion T=2", "white"):
            m, s = split[k], serial[k]
            assert (m.lmax_local, m.mmax_local, m.nlat_local, m.nlon_local) == (ll, ml, hl, wl)
            cut = s.sigma_l[:, :, :, l0:l0 + ll] if k != "white" else s.sigma_l[..., l0:l0 + ll, mo:mo + ml]
            assert torch.equal(m.sigma_l, cut), (rank, k, "sigma_l")
            if k != "white":
                assert torch.equal(m.phi, s.phi)
            assert tuple(m.state.shape) == (B, m.num_time_steps, C, ll, ml, 2)
            for stage, ((state, field), (wstate, wfield)) in enumerate(zip(_run(m), want[k])):
                assert bool(state.any()) and torch.equal(state, wstate[spec]), (rank, k, stage, "state")
                assert tuple(field.shape) == (B, m.num_time_steps, C, hl, wl) and bool(wfield[grid].abs().max() > 1e-3)
                e = rel(field, wfield[grid])
                print(f"h{h}w{w} rank {rank} {k} stage {stage}: field rel {e:.1e}", flush=True)
                assert e < TOL, (rank, k, stage, e)
            assert m.rng.tolist() == s.rng.tolist()

        # 7. the grid state of DummyNoiseS2
        d = split["dummy"]
        assert tuple(d.state.shape) == (B, 2, C, hl, wl)
        for stage, ((state, field), (wstate, _)) in enumerate(zip(_run(d), want["dummy"])):
            assert bool(state.any()) and torch.equal(state, wstate[grid]) and torch.equal(field, state), (rank, "dummy", stage)

        # 8. learnable white noise: autograd through the distributed inverse transform.  sigma_l is sharded over h AND w
        # (sharded_dims_mp), so no other rank shares a shard and the group to reduce over is this rank alone; the entries with
        # m > l do not enter the transform and their gradient is unspecified, as in the test of the transform itself
        ml_ = split["white learnable"]
        assert isinstance(ml_.sigma_l, torch.nn.Parameter) and ml_.sigma_l.sharded_dims_mp == [None, None, None, "h", "w"]
        assert torch.equal(ml_.sigma_l.detach(), sl.sigma_l.detach()[..., l0:l0 + ll, mo:mo + ml])
        ml_.update()
        assert torch.equal(ml_.state, sl.state[spec])
        (grad,) = torch.autograd.grad((ml_() * G[grid]).sum(), ml_.sigma_l)
        tri = torch.tril(torch.ones(37, 37, device=dev))[l0:l0 + ll, mo:mo + ml]
        e = rel(grad * tri, want_grad[..., l0:l0 + ll, mo:mo + ml] * tri)
        print(f"h{h}w{w} rank {rank} sigma_l gradient rel {e:.1e} (all entries: {rel(grad, want_grad[..., l0:l0 + ll, mo:mo + ml]):.1e})",
              flush=True)
        assert e < TOL and bool(want_grad.abs().max() > 1e-3), (rank, "sigma_l gradient", e)        # (a shard may lie wholly in m > l)

        # 9. saved generator and tensor state, restored into a fresh module on the same rank, continue bit-identically
        m = split["diffusion T=2"]
        rng_state, tensor_state = m.get_rng_state(), m.get_tensor_state()
        assert tuple(tensor_state.shape) == (B, 2, C, ll, ml, 2) and rng_state[1].tolist() == [12, 4]
        m.update()
        m.update()
        fresh = ma.DiffusionNoiseS2(IMG, 1, C, num_time_steps=2, kT=m.kT, lambd=m.lambd, seed=99, reflect=True).to(dev)
        fresh.set_rng_state(*rng_state)
        fresh.set_tensor_state(tensor_state)
        fresh.update()
        fresh.update()
        assert torch.equal(fresh.state, m.state) and fresh.rng.tolist() == m.rng.tolist() == [12, 6]
        torch.backends.cuda.matmul.allow_tf32 = was


@pytest.mark.parametrize("h,w", [(2, 1), (1, 2), (2, 2)])
def test_noise_shards_equal_the_serial_state_and_field(h, w):
    """DiffusionNoiseS2 (T = 1, 2), IsotropicGaussianRandomFieldS2 (fixed and learnable) and DummyNoiseS2 under h x w: states,
    sigma_l shards, fields, the sigma_l gradient and a save / restore, every rank against the serial module of the same seed"""
    launch(_worker, h * w, h, w, limit=240)
