"""The device path of the per-object spectra, as far as it goes without a GPU: the new entry point in the header, the binding and
the library, its switch, the packing of the SED library and the unchanged host path of instcat.to_catalog."""
import ctypes
import os
import re

import numpy as np

from imsim_amd import _abi, configs, instcat, sed as sedmod, tables, tuning

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_entry_point_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "imsim_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int\s+ims_object_spectra\(", header, re.M)
    assert re.search(r"#define IMS_ABI_VERSION 22\b", header)
    assert "ims_object_spectra" in _abi.EXPORTS
    lib = ctypes.CDLL(_abi.lib_path())                        # (no GPU needed: nothing is launched)
    assert lib.ims_abi_version() == 22
    assert lib.ims_object_spectra is not None
    assert len(_abi.load().ims_object_spectra.argtypes) == 20


def test_switch_is_known_and_off_by_default(monkeypatch):
    monkeypatch.delenv("IMS_SED_DEVICE", raising=False)
    assert "IMS_SED_DEVICE" in tuning.KNOWN and tuning.KNOWN["IMS_SED_DEVICE"][0] == "0"
    assert not tuning.flag("IMS_SED_DEVICE")
    with tuning.scoped(IMS_SED_DEVICE="1"):
        assert tuning.flag("IMS_SED_DEVICE")
    assert not tuning.flag("IMS_SED_DEVICE")


def _write_sed(path, wave, flam):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savetxt(path, np.column_stack([wave, flam]))


def test_pack_library_offsets_ids_order_and_missing(tmp_path):
    shapes = {"c.txt": np.linspace(300.0, 1200.0, 7), "a.txt": np.linspace(250.0, 900.0, 4), "sub/b.txt": np.linspace(400.0, 1000.0, 11)}
    for name, w in shapes.items():
        _write_sed(str(tmp_path / name), w, 1.0 + 0.001 * w)
    lib = sedmod.SedLibrary(str(tmp_path), None)
    names = ["c.txt", "nope.txt", "a.txt", "sub/b.txt", "c.txt", "a.txt", "nope.txt"]
    wave, fphot, offset, sed_id, missing = sedmod.pack_library(lib, names)
    # ids follow the sorted names of the files that were found: a.txt, c.txt, sub/b.txt
    assert missing == ["nope.txt"]
    assert offset.dtype == np.int64 and list(offset) == [0, 4, 11, 22]
    assert sed_id.dtype == np.int32 and list(sed_id) == [1, -1, 0, 2, 1, 0, -1]
    assert wave.dtype == np.float64 and fphot.dtype == np.float64 and len(wave) == len(fphot) == 22
    for k, name in enumerate(["a.txt", "c.txt", "sub/b.txt"]):
        s = lib.get(name)
        assert np.array_equal(wave[offset[k]:offset[k + 1]], s.wave) and np.array_equal(fphot[offset[k]:offset[k + 1]], s.fphotons)
    # nothing found at all: an empty library, every object missing
    wave, fphot, offset, sed_id, missing = sedmod.pack_library(lib, ["x", "y", "x"])
    assert len(wave) == len(fphot) == 0 and list(offset) == [0] and list(sed_id) == [-1, -1, -1] and missing == ["x", "y"]


def test_extinction_terms_are_the_curve():
    w = np.linspace(100.0, 3400.0, 500)                      # all four branches of the curve
    a, b = sedmod.ccm89_terms(w)
    for rv in (2.0, 3.1, 5.5):
        assert np.array_equal(sedmod.ccm89(w, rv), a + b / rv)


GALAXY = ("object 61441544815642 53.0091385 -27.4389488 24.8 galaxySED/g.txt 1.3 0.01 -0.02 0.003 0 0 "
          "sersic2d 0.5 0.3 20.0 1 CCM 0.2 2.7 CCM 0.02 3.1\n")
STAR = "object 1605472734212 53.0 -27.5 23.9 starSED/s.txt 0 0 0 0 0 0 point none CCM 0.03 3.1\n"


def test_to_catalog_without_sed_device_returns_numpy_tables(tmp_path):
    w = np.linspace(100.0, 2000.0, 381)
    _write_sed(str(tmp_path / "sed" / "galaxySED" / "g.txt"), w, np.exp(-0.5 * ((w - 400.0) / 300.0) ** 2))
    _write_sed(str(tmp_path / "sed" / "starSED" / "s.txt"), w, 1.0 + 0.0 * w)
    f = tmp_path / "cat.txt"
    f.write_text(GALAXY + STAR + STAR.replace("starSED/s.txt", "starSED/none.txt").replace("1605472734212", "5"))
    p = instcat.parse_objects(str(f))
    wl, thr = tables.synthetic_r_band()
    o = configs.rubin_optics_struct(4096, 4096)
    cat = instcat.to_catalog(p, o.img_wcs, 4096, 4096, float(np.trapezoid(thr, wl)), 30.0, sed_dir=str(tmp_path / "sed"),
                             bandpass=(wl, thr), sed_points=129, sort_mag=False, edge_pix=10 ** 7)
    assert isinstance(cat["sed_tables"], np.ndarray) and cat["sed_tables"].shape == (2, 129) and cat["sed_tables"].dtype == np.float64
    assert cat["missing_seds"] == ["starSED/none.txt"] and list(cat["sed_table"]) == [1, 2, 0]
    # the rows are what the host function gives for those objects
    names = [s[0] for s in p["sed"]]
    z = np.array([s[1] for s in p["sed"]])
    f0, tabs, _ = sedmod.object_spectra(names, z, p["dust"][:, 2], p["dust"][:, 3], wl, thr, sedmod.SedLibrary(str(tmp_path / "sed"), None),
                                        n_pts=129)
    assert np.array_equal(cat["sed_tables"], tabs[:2])
    assert "sed_device" in instcat.to_catalog.__code__.co_varnames
