"""ims_object_spectra / sed.object_spectra_hip against the unchanged host sed.object_spectra on the same inputs, and the device
tables through the engine, instcat.to_catalog and config.Process.

Bounds (derived, not tuned): two differently ordered sums of at most 1 601 positive terms differ by at most about 2e-13
relative and exp by a few ulp, so
  flux            1e-12 relative; exactly -1 and exactly 0 where the host gives those
  rows            non-decreasing, inside [lo, hi], exactly lo at j = 0
  CDF             |C_ref(lambda_gpu[j]) - u_j| <= 1e-11, C_ref the host's normalised CDF through its kept knots
  wavelengths     1e-6 nm in qualifying brackets = step * 2e-13 / 1e-6 with ten times margin: the host bracket is two adjacent
                  grid points that hold at least 1e-6 of the normalised mass, and neither is the first or last point of
                  positive density
  share           qualifying entries are at least 95 % of the entries of the objects with positive flux.  The entries j = 0 and
                  j = n_pts - 1 of every row lie in the first and the last bracket of positive density and never qualify, so
                  a case of 33-point tables alone cannot pass 31 / 33 = 93.9 %: the share is taken over the entries of all
                  cases together (and printed per case).
"""
import gzip
import os

import numpy as np
import pytest

from imsim_amd import _abi, catalog, config, configs, sed as sedmod, tables, tuning
from imsim_amd.engine import Renderer
from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INSTCAT = os.path.join(HERE, "golden", "example_instcat_subset.txt")
STEP = 0.5
SED_NAMES = ["bb.txt", "line.txt", "two.txt", "short.txt"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def planck_flambda(w, temp=5500.0):
    return 1.0e15 / w ** 5 / np.expm1(1.43877688e7 / (w * temp))


def write_seds(d):
    """a smooth black body (3 801 points), the same with a narrow top-hat emission line, a 2-point SED, and one that is zero
    below 560 nm (but for the normalisation wavelength) and ends at 650 nm: plateaus at both ends of a 540 - 692 nm band at z = 0"""
    w = 100.0 + 0.5 * np.arange(3801)
    bb = planck_flambda(w)
    np.savetxt(os.path.join(d, "bb.txt"), np.column_stack([w, bb]))
    np.savetxt(os.path.join(d, "line.txt"), np.column_stack([w, bb * np.where((w >= 310.0) & (w <= 311.0), 6.0, 1.0)]))
    np.savetxt(os.path.join(d, "two.txt"), np.array([[300.0, 1.0], [1200.0, 2.5]]))
    ws = 450.0 + 0.25 * np.arange(801)
    np.savetxt(os.path.join(d, "short.txt"), np.column_stack([ws, planck_flambda(ws, 4000.0) * ((ws >= 560.0) | (np.abs(ws - 500.0) < 5.0))]))
    return d


def band(lo, hi, edge):
    """a throughput with raised-cosine edges `edge` nm wide: smooth, and no long tails"""
    wl = np.append(np.arange(lo, hi, 0.1), hi)
    t = np.minimum(np.minimum((wl - lo) / edge, (hi - wl) / edge), 1.0)
    return wl, 0.6 * 0.5 * (1.0 - np.cos(np.pi * t)) * (1.0 - 0.0005 * (wl - lo))


def make_objects(n, seed, z_max=3.0):
    """names in arbitrary order with an absent one among them, redshifts 0 .. z_max, A_v 0 and 3, R_v 3.1 and 2.0 mixed"""
    rng = np.random.default_rng(seed)
    names = np.array(SED_NAMES + ["absent.txt"], dtype=object)[rng.integers(0, 5, n)]
    z = np.round(rng.uniform(0.0, z_max, n), 3)
    av = np.where(rng.random(n) < 0.5, 0.0, 3.0)
    rv = np.where(rng.random(n) < 0.5, 3.1, 2.0)
    fixed = [("short.txt", 3.0, 0.0, 3.1),                    # 1 800 - 2 600 nm: wholly out of any band here
             ("short.txt", 0.0, 3.0, 2.0), ("two.txt", 0.0, 0.0, 3.1), ("absent.txt", 0.5, 3.0, 3.1), ("line.txt", 1.0, 0.0, 2.0)]
    for k, (nm, zz, a, r) in enumerate(fixed[:n]):
        names[k], z[k], av[k], rv[k] = nm, zz, a, r
    return names, z, av, rv


# (band lo, hi, edge width, n_pts, objects, lead_rows, seed)
CASES = {
    "uneven_last_step_300": (540.0, 692.3, 12.0, 257, 300, 1, 1),      # n_grid = 306: no multiple of 64, last step 0.3 nm
    "five_objects_129": (540.0, 692.3, 12.0, 129, 5, 0, 2),            # the last workgroup partly empty
    "narrow_band_33": (600.0, 610.0, 2.0, 33, 40, 0, 3),               # n_grid = 21 < 64
    "full_grid_1601": (300.0, 1100.0, 40.0, 257, 70, 1, 4),            # the largest grid the kernel takes; 25 segments per lane
    "uneven_33": (540.0, 692.3, 12.0, 33, 31, 1, 5),
}


def host_cdf(name, z, av, rv, wl, thr, library):
    """sed.object_spectra's arithmetic for one object: (grid, density, cumulative sum)"""
    lo, hi = float(wl[0]), float(wl[-1])
    grid = np.arange(lo, hi + 0.5 * STEP, STEP)
    grid[-1] = min(grid[-1], hi)
    t = np.interp(grid, wl, thr, left=0.0, right=0.0)
    s = library.get(name)
    spec = np.interp(grid[None, :] / (1.0 + np.array([z])[:, None]), s.wave, s.fphotons, left=0.0, right=0.0)
    dens = spec * sedmod.extinction_factor(grid, np.array([av]), np.array([rv])) * t[None, :]
    seg = 0.5 * (dens[:, 1:] + dens[:, :-1]) * np.diff(grid)[None, :]
    return grid, dens[0], np.concatenate([np.zeros((1, 1)), np.cumsum(seg, axis=1)], axis=1)[0]


def check_case(key, objs, wl, thr, library, n_pts, flux, tabs, missing, ref):
    """every criterion of the module docstring but the share; returns (qualifying entries, entries of positive-flux objects)"""
    names, z, av, rv = objs
    rflux, rtabs, rmissing = ref
    lo, hi = float(wl[0]), float(wl[-1])
    assert missing == rmissing and ("absent.txt" in missing) == ("absent.txt" in set(names.tolist()))
    assert np.array_equal(flux == -1.0, rflux == -1.0) and np.array_equal(flux == 0.0, rflux == 0.0)
    pos = rflux > 0.0
    rel = np.abs(flux[pos] / rflux[pos] - 1.0)
    print(f"{key}: {len(names)} objects, {int(pos.sum())} with flux, {int((rflux == 0).sum())} out of band, {int((rflux < 0).sum())} absent; "
          f"flux max rel {rel.max() if rel.size else 0.0:.3g}")
    assert np.all(rel <= 1e-12)
    assert np.array_equal(tabs[rflux < 0.0], np.zeros((int((rflux < 0.0).sum()), n_pts)))
    assert np.array_equal(tabs[rflux == 0.0], rtabs[rflux == 0.0])          # np.linspace(lo, hi, n_pts)
    ok = rflux >= 0.0
    assert np.all(np.diff(tabs[ok], axis=1) >= 0.0) and tabs[ok].min() >= lo and tabs[ok].max() <= hi and np.all(tabs[ok][:, 0] == lo)
    u = np.linspace(0.0, 1.0, n_pts)
    n_qual = n_all = 0
    worst_c = worst_w = 0.0
    for i in np.flatnonzero(pos):
        grid, dens, c = host_cdf(names[i], z[i], av[i], rv[i], wl, thr, library)
        assert c[-1] == rflux[i]                                # the same arithmetic as the reference's
        c = c / c[-1]
        keep = np.concatenate([[True], np.diff(c) > 0])
        xk, gk, ik = c[keep], grid[keep], np.flatnonzero(keep)
        assert np.array_equal(np.interp(u, xk, gk), rtabs[i])
        worst_c = max(worst_c, float(np.abs(np.interp(tabs[i], gk, xk) - u).max()))
        # the host bracket of every entry: kept knots j, j + 1 with xk[j] <= u < xk[j + 1] (u = 1: the last interval)
        j = np.clip(np.searchsorted(xk, u, side="right") - 1, 0, len(xk) - 2)
        nz = np.flatnonzero(dens > 0.0)
        qual = ((ik[j + 1] - ik[j] == 1) & (xk[j + 1] - xk[j] >= 1e-6)
                & ~np.isin(ik[j], (nz[0], nz[-1])) & ~np.isin(ik[j + 1], (nz[0], nz[-1])))
        if qual.any():
            worst_w = max(worst_w, float(np.abs(tabs[i] - rtabs[i])[qual].max()))
        n_qual += int(qual.sum())
        n_all += n_pts
    print(f"{key}: max |C_ref(lambda) - u| {worst_c:.3g}; max |d lambda| in qualifying brackets {worst_w:.3g} nm; "
          f"qualifying {n_qual} of {n_all} entries ({n_qual / max(n_all, 1):.4f})")
    assert worst_c <= 1e-11
    assert worst_w <= 1e-6
    return n_qual, n_all


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return sedmod.SedLibrary(write_seds(str(tmp_path_factory.mktemp("seds"))), None)


def case_inputs(key):
    lo, hi, edge, n_pts, n, lead, seed = CASES[key]
    wl, thr = band(lo, hi, edge)
    return wl, thr, n_pts, lead, make_objects(n, seed)


@pytest.fixture(scope="module")
def shares():
    return {}


@pytest.mark.parametrize("key", list(CASES))
def test_device_spectra_against_the_host(torch_cuda, library, shares, key):
    torch = torch_cuda
    wl, thr, n_pts, lead, objs = case_inputs(key)
    names, z, av, rv = objs
    ref = sedmod.object_spectra(names, z, av, rv, wl, thr, library, n_pts=n_pts, step=STEP)
    out = torch.full((lead + len(names), n_pts), -7.25, dtype=torch.float64, device="cuda:0") if lead else None
    flux, tabs, missing = sedmod.object_spectra_hip(names, z, av, rv, wl, thr, library, n_pts=n_pts, step=STEP, device="cuda:0",
                                                    lead_rows=lead, out=out)
    assert isinstance(flux, np.ndarray) and flux.dtype == np.float64 and flux.shape == (len(names),)
    assert torch.is_tensor(tabs) and tabs.is_cuda and tabs.dtype == torch.float64 and tuple(tabs.shape) == (lead + len(names), n_pts)
    t = tabs.cpu().numpy()
    if lead:
        assert tabs.data_ptr() == out.data_ptr() and np.all(t[:lead] == -7.25), "the caller's leading rows were touched"
        fresh = sedmod.object_spectra_hip(names, z, av, rv, wl, thr, library, n_pts=n_pts, step=STEP, device="cuda:0", lead_rows=lead)[1]
        assert np.all(fresh[:lead].cpu().numpy() == 0.0) and np.array_equal(fresh[lead:].cpu().numpy(), t[lead:])
    if key == "uneven_last_step_300":
        grid = sedmod.band_grid(wl, thr, STEP)[2]
        assert len(grid) == 306 and abs((grid[-1] - grid[-2]) - 0.3) < 1e-9
        assert ref[0][0] == 0.0 and np.array_equal(t[lead], np.linspace(wl[0], wl[-1], n_pts))     # short.txt at z = 3
    shares[key] = check_case(key, objs, wl, thr, library, n_pts, flux, t[lead:], missing, ref)


def test_share_of_qualifying_entries(torch_cuda, shares):
    """runs behind the cases above (file order) and needs them all"""
    assert set(shares) == set(CASES), "the cases did not all run"
    n_qual, n_all = (sum(v[k] for v in shares.values()) for k in (0, 1))
    print(f"qualifying entries: {n_qual} of {n_all} ({n_qual / n_all:.4f})")
    assert n_qual >= 0.95 * n_all


def test_grid_that_does_not_fit_is_refused(torch_cuda, library):
    wl, thr = band(300.0, 1400.0, 40.0)                        # 2 201 points
    with pytest.raises(_abi.ImsimHipError, match="does not fit"):
        sedmod.object_spectra_hip(["bb.txt"], [0.0], [0.0], [3.1], wl, thr, library, device="cuda:0")


def test_renderer_reads_the_device_tables_in_place(torch_cuda, library):
    """the same scene rendered from the device tensor and from its host copy: the same bits"""
    torch = torch_cuda
    wl, thr = tables.synthetic_r_band()
    n = 50
    names, z, av, rv = make_objects(n, 11, z_max=1.0)
    names[names == "absent.txt"] = "bb.txt"
    flux, tabs, _ = sedmod.object_spectra_hip(names, z, av, rv, wl, thr, library, device="cuda:0", lead_rows=1)
    tabs[0].copy_(torch.from_numpy(tables.inverse_cdf_table(wl, thr, n_pts=tabs.shape[1])))
    torch.cuda.synchronize()
    assert np.all(flux >= 0.0)
    images = []
    for sed_tables in (tabs, tabs.cpu().numpy()):
        scene = configs.scene_c3(nx=256, ny=256)
        scene.sensor.scratch_cells = 400_000
        scene.sed_tables = sed_tables
        cat = catalog.synthetic_catalog(n, nx=256, ny=256)
        cat["sed_table"] = np.where(flux > 0.0, 1 + np.arange(n), 0).astype(np.int32)
        phot = catalog.realize_fluxes(cat["nominal_flux"], 7)
        objects, _ = configs.c3_objects(cat, phot, scene)
        r = Renderer(scene, "cuda:0", lazy_static=True)
        if sed_tables is tabs:
            sed = r.bound.base_params.sed
            assert sed.val == tabs.data_ptr() and (sed.n_tables, sed.n_pts) == tuple(tabs.shape)
        r.render_lsst_image(objects, nrecalc=1000)
        r.synchronize()
        images.append(r.image_numpy())
    assert images[0].sum() > 0
    assert_bits_equal(images[0], images[1], "device tensor against its host copy")
    # and the tables matter to the image: with the flat fallback for everyone it is another image
    scene = configs.scene_c3(nx=256, ny=256)
    scene.sensor.scratch_cells = 400_000
    cat = catalog.synthetic_catalog(n, nx=256, ny=256)
    phot = catalog.realize_fluxes(cat["nominal_flux"], 7)
    objects, _ = configs.c3_objects(cat, phot, scene)
    r = Renderer(scene, "cuda:0", lazy_static=True)
    r.render_lsst_image(objects, nrecalc=1000)
    r.synchronize()
    assert not np.array_equal(r.image_numpy(), images[0])


def test_process_with_the_switch_on_and_off(torch_cuda, tmp_path):
    """config.Process on the example catalog with a synthetic sed_dir (one file left out): the same objects, nominal fluxes
    within 1e-12 and the same missing SEDs either way.  The images are not compared: the photon wavelengths differ in their
    last bits by design."""
    with open(INSTCAT) as f:
        names = [ln.split()[5] for ln in f if ln.startswith("object")]
    names = [names[0]] + sorted(set(names) - {names[0]})        # the first object's SED (four of the first twelve objects have it)
    sed_dir = tmp_path / "sed"
    w = 100.0 + 10.0 * np.arange(191)                           # (128 files: coarse ones keep the test quick)
    for k, name in enumerate(names[1:]):                        # the first name stays absent
        p = sed_dir / name
        p.parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(p, "wt") as f:
            np.savetxt(f, np.column_stack([w, planck_flambda(w, 3000.0 + 500.0 * (k % 9))]))
    results = []
    for on in ("0", "1"):
        over = {"input.instance_catalog.file_name": INSTCAT, "input.instance_catalog.sed_dir": str(sed_dir), "stamp.draw_method": "phot",
                "output.dir": str(tmp_path / on), "image.nobjects": 12}
        with tuning.scoped(IMS_SED_DEVICE=on):
            results.append(config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                                          overrides=over))
    off, dev = results
    miss = [[s for s in r.ignored if "SED file(s) not found" in s] for r in results]
    print("missing:", miss[0])
    assert miss[0] == miss[1] and len(miss[0]) == 1 and names[0] in miss[0][0]
    t0, t1 = off.truth[0], dev.truth[0]
    assert len(t0["object_id"]) == 12 and list(t0["object_id"]) == list(t1["object_id"])
    assert np.array_equal(t0["x"], t1["x"]) and np.array_equal(t0["y"], t1["y"])
    rel = np.abs(np.asarray(t1["nominal_flux"]) / np.asarray(t0["nominal_flux"]) - 1.0)
    print("nominal_flux max rel:", rel.max(), "objects:", len(rel))
    assert np.all(rel <= 1e-12)
    assert dev.images[0].sum() > 0 and dev.images[0].shape == off.images[0].shape
