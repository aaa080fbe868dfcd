"""FourCastNet3.1 (makani_amd/fcn31.py) against fixtures written by the reference's own ``AtmoSphericNeuralOperatorNet31``
(``tools/make_golden_fcn31.py``): constructor / state-dict / index-buffer contract and errors on the CPU, forward + every gradient on
the GPU — fp32 end to end 1e-4 on the output and the input gradient, parameter gradients 2e-4 or within 1e-4 of the largest gradient
magnitude (the gates of tests/test_fcn3.py); bf16 autocast 4e-2 / 8e-2 against the fp32 fixture.

  fcn31_small_33x64     B = 1, morlet, sst + xlsml (land mask read from x), position embedding, instance norm, big skip, water clamp
  fcn31_history_24x48   B = 2, n_history = 1, layer norm, sin, encoder bias, no xlsml (NaN-only mask), two imputed channels
  fcn31_nomlp_24x48     use_mlp=False (the convolutions change width), no layer scale, SHT resampling, no sst, clamp offsets"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_l2

FIXTURES = ["fcn31_small_33x64", "fcn31_history_24x48", "fcn31_nomlp_24x48"]
SMALL = dict(inp_shape=(16, 32), out_shape=(16, 32), scale_factor=2, filter_basis_type="morlet", hard_thresholding_fraction=1.0)


def _load(name):
    import makani_amd as ma
    g = load_golden(name + ".npz")
    kwargs = json.loads(str(g["kwargs"]))
    model = ma.AtmoSphericNeuralOperatorNet31(**kwargs, some_unknown_trainer_key=1)       # unknown kwargs are ignored
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    model.load_state_dict(sd, strict=True)
    return g, kwargs, model


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_and_index_buffers_are_the_reference_s(name):
    g, kwargs, model = _load(name)
    ref = {k[len("param/"):]: tuple(g[k].shape) for k in g.files if k.startswith("param/")}
    own = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert own == ref and list(own) == list(ref)
    assert set(dict(model.named_parameters())) == {k[len("grad/"):] for k in g.files if k.startswith("grad/")}
    recorded = {k[len("buffer/"):]: g[k] for k in g.files if k.startswith("buffer/")}
    assert {"in_channels", "aux_channels", "pred_channels", "sst_channels_in", "land_mask_channels", "atmo_channels_in"} <= set(recorded)
    for k, v in recorded.items():
        b = getattr(model, k)
        assert b.dtype == torch.long and b.tolist() == v.tolist(), k
        assert k not in own          # non-persistent
    for k, p in model.named_parameters():
        if "layer_scale" in k or ".mlp.fwd." in k:
            assert getattr(p, "is_shared_mp", None) == ["spatial"], k
        if k.endswith("global_conv.weight"):
            assert p.is_shared_mp == ["matmul", "w"] and p.sharded_dims_mp[-1] == "h", k
        if k == "pos_embed.position_embeddings":
            assert p.is_shared_mp == ["w"] and p.sharded_dims_mp == [None, None, "h", None]
    assert model.n_out_chans == len(kwargs["channel_names"]) and model.n_history == kwargs.get("n_history", 0)
    assert hasattr(model, "sst_imputation") == ("sst" in kwargs["channel_names"])


def test_fixture_contents():
    g, kw, m = _load("fcn31_small_33x64")
    assert len([k for k in g.files if k.startswith("param/")]) == 47 and g["x"].shape[0] == 1 and m.lmax == 16 == m.sht.mmax
    assert m.sst_imputation.mask_channel == m.land_mask_channels.item() == 13 + 2 and np.isnan(g["x"][:, 12]).any()
    assert (g["gx"][np.isnan(g["x"])] == 0).all() and not np.isnan(g["y"]).any() and np.abs(g["param/pos_embed.position_embeddings"]).max() > 0
    g, kw, m = _load("fcn31_history_24x48")
    assert g["x"].shape[:2] == (2, 23) and m.sst_channels_in.tolist() == [9, 9 + 11] and m.sst_imputation.mask_channel is None
    assert m.in_channels.numel() == 20 and m.stat_aux_channels.tolist() == [10 + 11 + 1] and np.isnan(g["x"][:, 20]).any()
    g, kw, m = _load("fcn31_nomlp_24x48")
    assert not hasattr(m, "sst_imputation") and "normalization_means" in m.state_dict() and m.water_channels.tolist() == [3, 7, 11]
    assert tuple(m.blocks[1].local_conv.weight.shape)[:2] == (8, 12) and not hasattr(m.blocks[0], "mlp")          # 12 -> 8 channels


def test_helpers():
    from makani_amd import fcn31
    assert fcn31.compute_spherical_bandlimit((721, 1440), "equiangular") == 360 and fcn31.compute_spherical_bandlimit((360, 720), "legendre-gauss") == 359
    assert fcn31._compute_cutoff_radius(lmax=120, kernel_shape=(3, 3), basis_type="morlet") == pytest.approx(3 * np.pi / 120)
    m = fcn31.AtmoSphericNeuralOperatorNet31(**SMALL, lmax=5, num_layers=1)
    assert m.lmax == 5 == m.sht.lmax == m.isht.mmax
    e = fcn31.LearnablePositionEmbedding((6, 12), num_chans=3, embed_type="latlon")
    assert tuple(e.position_embeddings.shape) == (1, 3, 6, 12) and e.position_embeddings.is_shared_mp == [] \
        and e.position_embeddings.sharded_dims_mp == [None, None, "h", "w"] and tuple(e().shape) == (1, 3, 6, 12)
    e = fcn31.LearnablePositionEmbedding((6, 12), num_chans=3)
    assert tuple(e.position_embeddings.shape) == (1, 3, 6, 1) and tuple(e().shape) == (1, 3, 6, 12)


def test_errors():
    from makani_amd import fcn31
    with pytest.raises(ValueError, match="Unknown activation function tanh"):
        fcn31.AtmoSphericNeuralOperatorNet31(**SMALL, activation_function="tanh")
    with pytest.raises(ValueError):          # unequal level groups
        fcn31.AtmoSphericNeuralOperatorNet31(**SMALL, channel_names=["u500", "v500", "u850"])
    for basis in ("harmonic", "fourier-bessel"):
        with pytest.raises(NotImplementedError, match="no torch-harmonics release"):
            fcn31.AtmoSphericNeuralOperatorNet31(**dict(SMALL, filter_basis_type=basis))
    with pytest.raises(NotImplementedError, match="nodal"):
        fcn31.AtmoSphericNeuralOperatorNet31(**SMALL, filter_basis_norm_mode="nodal")
    with pytest.raises(NotImplementedError, match="no torch-harmonics release"):          # the sub-classes' own defaults
        fcn31.DiscreteContinuousEncoder(inp_shape=(16, 32), out_shape=(8, 16), lmax=7)
    with pytest.raises(ValueError, match="Unknown learnable position embedding type grid"):
        fcn31.LearnablePositionEmbedding((6, 12), embed_type="grid")
    with pytest.raises(NotImplementedError, match="at most 256 channels"):          # the imputation's capacities
        fcn31.AtmoSphericNeuralOperatorNet31(**SMALL, channel_names=[f"u{p}" for p in range(100, 360)] + ["sst"])
    with pytest.raises(NotImplementedError, match="Unknown type"):
        fcn31.compute_spherical_bandlimit((8, 16), "lobatto")


def test_plugin_exports():
    import makani_amd as ma
    import makani_plugin
    assert makani_plugin.AtmoSphericNeuralOperatorNet31 is ma.AtmoSphericNeuralOperatorNet31 and callable(makani_plugin.register_fcn31)
    assert 'nettype: "/path/to/repo/makani_plugin.py:AtmoSphericNeuralOperatorNet31"' in makani_plugin.__doc__


def test_fixture_provenance():
    """where the reference is present its own class, run again, gives the stored arrays of fcn31_history_24x48"""
    sys.path.insert(0, ROOT)
    from oracle import ref_shims
    if not ref_shims.reference_available():
        pytest.skip("no reference checkout: the fixture cannot be regenerated here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_fcn31
    g = load_golden("fcn31_history_24x48.npz")
    fresh = make_golden_fcn31.network_case("fcn31_history_24x48")
    assert set(fresh) == set(g.files)
    for k, v in fresh.items():
        if k == "kwargs":
            assert json.loads(str(v)) == json.loads(str(g[k]))
        elif k in ("x", "g") or k.startswith("buffer/") or k.startswith("param/"):
            assert np.array_equal(v, g[k], equal_nan=True), k
        else:
            assert rel_l2(torch.from_numpy(np.asarray(v)), torch.from_numpy(g[k])) < 1e-5, k


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------
def _run(model, g, amp=False):
    x = torch.from_numpy(g["x"]).to("cuda:0").requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        y = model(x)
    (y.float() * torch.from_numpy(g["g"]).to("cuda:0")).sum().backward()
    return x, y


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_matches_reference_golden_fp32(name):
    g, kwargs, model = _load(name)
    model = model.to("cuda:0")
    x, y = _run(model, g)
    nan = torch.from_numpy(np.isnan(g["x"]))
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and (x.grad.cpu()[nan] == 0).all()
    e_y, e_gx = rel_l2(y, torch.from_numpy(g["y"])), rel_l2(x.grad, torch.from_numpy(g["gx"]))
    print(f"FourCastNet3.1 {name} fp32: output {e_y:.2e}, input gradient {e_gx:.2e}")
    assert e_y < 1e-4 and e_gx < 1e-4
    gmax = max(float(np.abs(g[k2]).max()) for k2 in g.files if k2.startswith("grad/"))
    worst = 0.0
    for k, p in model.named_parameters():
        ref = torch.from_numpy(g["grad/" + k])
        assert p.grad is not None and torch.isfinite(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).all(), k
        e = rel_l2(p.grad, ref)
        a = (torch.view_as_real(p.grad.detach().cpu()) - torch.view_as_real(ref)).abs().max().item() if ref.is_complex() else \
            (p.grad.detach().cpu() - ref).abs().max().item()
        assert e < 2e-4 or a < 1e-4 * gmax, (k, e, a, gmax)        # zero-in-exact-arithmetic gradients: absolute scale
        worst = max(worst, e)
    print(f"    largest parameter-gradient rel-L2: {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_autocast_runs_close_to_fp32(name):
    g, kwargs, model = _load(name)
    model = model.to("cuda:0")
    x, y = _run(model, g, amp=True)
    e_y, e_gx = rel_l2(y.float(), torch.from_numpy(g["y"])), rel_l2(x.grad, torch.from_numpy(g["gx"]))
    print(f"FourCastNet3.1 {name} bf16 autocast vs the fp32 fixture: output {e_y:.2e}, input gradient {e_gx:.2e}")
    assert e_y < 4e-2 and e_gx < 8e-2
    assert all(p.grad is not None and torch.isfinite(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).all()
               for p in model.parameters())


@pytest.mark.gpu
def test_fused_stages_equal_the_composed_methods_and_batch_expansion():
    """forward's two fused launches against the public composed methods on the same model; the position embedding over B = 3"""
    g, kwargs, model = _load("fcn31_small_33x64")
    model = model.to("cuda:0")
    x = torch.from_numpy(g["x"]).to("cuda:0").repeat(3, 1, 1, 1)
    with torch.no_grad():
        xi = model.impute_sst_channels(x)
        assert torch.equal(xi, model.sst_imputation(x)) and torch.isfinite(xi).all()
        d = model.decode(model.processor_blocks(model.encode(xi), model.encode_auxiliary_channels(xi)))
        composed = model.clamp_water_channels(d + xi[..., model.pred_channels, :, :])
        y = model(x)
    assert y.shape[0] == 3 and rel_l2(y, composed) < 1e-6 and rel_l2(y[2], torch.from_numpy(g["y"])[0]) < 1e-4
