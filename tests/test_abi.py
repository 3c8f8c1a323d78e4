"""CPU-only checks of the drop-in boundary: the C-ABI library builds, loads, and exports every
symbol include/periodhip.h declares; the host layer fails loudly without a GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ph_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    return _ffi.load()


def test_every_declared_symbol_is_exported(lib):
    from pyperiod_amd import _ffi

    names = _header_symbols()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in periodhip.h but not exported"
    assert sorted(list(_ffi.SIGNATURES) + ["ph_last_error", "ph_profile_name"]) == names
    assert lib.ph_version() == 100


def test_header_constants_match_binding():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    for name in ("PH_OK", "PH_E_ARG", "PH_E_HIP", "PH_E_NOMEM", "PH_E_CAP", "PH_E_UNSUPPORTED", "PH_F64", "PH_F32",
                 "PH_FLAG_TRUNC", "PH_FLAG_ORTH", "PH_FLAG_SINGLE", "PH_FLAG_DEVICE", "PH_FLAG_NOSYNC", "PH_SWEEP_NORM",
                 "PH_SWEEP_NORM_GAMMA", "PH_SWEEP_MAXABS", "PH_ST_OK", "PH_ST_NO_PERIOD", "PH_ST_ITER_CAP", "PH_ST_CAP",
                 "PH_QO_LDS_OVERLAY", "PH_QO_LDS_BEHIND", "PH_QO_HBM",
                 "PH_OP_PROJECT", "PH_OP_SWEEP", "PH_OP_M_BEST", "PH_OP_SMALL_TO_LARGE", "PH_OP_BEST_CORRELATION",
                 "PH_OP_BEST_FREQUENCY", "PH_OP_RAMANUJAN", "PH_OP_ORTH_POWERS", "PH_OP_FOLD_SUMS",
                 "PH_PLAN_KERNELS", "PH_PLAN_K0", "PH_PLAN_K1", "PH_PLAN_STRIDE", "PH_PLAN_LEN", "PH_PLAN_VARIANT",
                 "PH_PLAN_WINDOW", "PH_PLAN_SECOND", "PH_PLAN_BLOCK", "PH_PLAN_LDS_BYTES", "PH_PLAN_SMALL_MEANS",
                 "PH_PLAN_WAVES", "PH_PLAN_PAD", "PH_PLAN_ONE", "PH_PLAN_PAIR", "PH_PLAN_FFT", "PH_PLAN_CHIRP",
                 "PH_PLAN_DIRECT", "PH_PLAN_NONE", "PH_PLAN_LDS", "PH_PLAN_HBM"):
        m = re.search(rf"#define {name} \(?(-?\d+)u?\)?", text)
        assert m, name
        assert int(m.group(1)) == getattr(_ffi, name), name


def test_argument_errors_without_gpu(lib):
    from pyperiod_amd import _ffi

    # NULL context -> PH_E_ARG with a message, no crash, no GPU needed
    rc = lib.ph_sweep(None, None, 0, 1, 16, 2, 5, 0, None, None, 0, 0, None)
    assert rc == _ffi.PH_E_ARG
    assert b"ctx" in lib.ph_last_error()
    with pytest.raises(ValueError):
        _ffi.check(rc)


def test_helper_entry_points_reject_null_without_gpu(lib):
    """The round-2 helpers (pass-plan info, QOPeriods feasibility) validate their arguments on the host."""
    from pyperiod_amd import _ffi

    n_pass, n_per, ok = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(7)
    assert lib.ph_sweep_plan_info(None, 2, 1365, ctypes.byref(n_pass), ctypes.byref(n_per)) == _ffi.PH_E_ARG
    assert lib.ph_qo_feasible(None, _ffi.PH_F64, 4096, -1, 512, ctypes.byref(ok)) == _ffi.PH_E_ARG
    assert lib.ph_qo_plan_info(None, _ffi.PH_F64, 4096, -1, 512, 0, ctypes.byref(ok), ctypes.byref(ok)) == _ffi.PH_E_ARG
    rec = (ctypes.c_int32 * _ffi.PH_PLAN_LEN)()
    assert lib.ph_plan_info(None, _ffi.PH_OP_SWEEP, _ffi.PH_F64, 4096, None, 0, 0, ctypes.addressof(rec)) == _ffi.PH_E_ARG
    assert lib.ph_small_to_large(None, None, 0, 1, 16, 0.1, -1, None, None, 0, _ffi.PH_FLAG_DEVICE | _ffi.PH_FLAG_NOSYNC, 4,
                                 None, None, None, None, None) == _ffi.PH_E_ARG
    assert _ffi.PH_FLAG_NOSYNC == 16


def test_product_has_no_cpu_fallback(lib):
    """Without a GPU the class surface must raise, not compute on the host."""
    n = ctypes.c_int(0)
    lib.ph_device_count(ctypes.byref(n))
    if n.value > 0:
        pytest.skip("GPU present")
    from pyperiod_amd import Periods
    from pyperiod_amd._ffi import PeriodHipError

    with pytest.raises(PeriodHipError):
        Periods.project(np.arange(10.0), 3)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pyperiod_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "period_oracle" not in src and "import oracle" not in src and "from oracle" not in src, f


def test_set_order_tables_match_reference(golden):
    """The CSR tables fed to the kernels reproduce the reference's divisor-set iteration order."""
    from pyperiod_amd import _factors

    kat = golden("kat")
    off = kat["factor_order_off"]
    foff, fq = _factors.factor_tables(1399)
    ooff, oq = _factors.orth_tables(1399)
    for k, n in enumerate(kat["factor_order_n"]):
        want = [int(v) for v in kat["factor_order_flat"][off[k] : off[k + 1]]]
        assert list(fq[foff[n] : foff[n + 1]]) == want, n
        assert list(oq[ooff[n] : ooff[n + 1]]) == [n // f for f in want if f in _factors.PRIMES], n
    assert _factors.phi(9) == 6 and _factors.phi(10) == 4
    assert len(_factors.PRIMES) == 1229


def test_host_dictionaries_match_reference(golden):
    """Integer Ramanujan sums / natural-basis rows built on the host (no GPU involved)."""
    from pyperiod_amd.QOPeriods import QOPeriods, ramanujan_sum

    g = golden("ramanujan")
    for q in range(1, 65):
        assert np.array_equal(ramanujan_sum(q), np.rint(g[f"cq_{q}"]).astype(np.int64))
    gq = golden("qoperiods")
    assert np.array_equal(QOPeriods.Pp(5, 12, keep=3), gq["pp_5_12_keep3"])
    qo = QOPeriods()
    a, d = qo.get_subspaces([37, 64, 101], 256)
    assert list(d.values()) == [37, 63, 100] and a.shape == (200, 256)
    assert [int(k) for k in d] == list(gq["dims_37_64_101_keys"])
    from pyperiod_amd import RamanujanPeriods

    assert np.max(np.abs(RamanujanPeriods().Cq_complete(6, 20) - g["cq_complete_6_20"])) < 1e-12


def test_built_tree_builds_read_only(lib, tmp_path):
    """build() of an up-to-date tree writes nothing (no lock file, no library), so a tree built by another user
    imports for this one: the copy is made read-only (binding for a non-root user) and every file of it must be the
    same afterwards (binding for root too)."""
    import shutil
    import stat
    import subprocess
    import sys

    tree = tmp_path / "tree"
    skip = shutil.ignore_patterns("__pycache__", ".build.lock")
    for d in ("pyperiod_amd", "include"):
        shutil.copytree(os.path.join(ROOT, d), tree / d, ignore=skip)  # copy2: the library stays newer than its sources
    shutil.copy2(os.path.join(ROOT, "__graft_entry__.py"), tree)

    def files():
        return {str(p.relative_to(tree)): (p.stat().st_mtime_ns, p.stat().st_size) for p in tree.rglob("*") if p.is_file()}

    before = files()
    dirs = [tree] + [p for p in tree.rglob("*") if p.is_dir()]
    for p in dirs:
        p.chmod(stat.S_IRUSR | stat.S_IXUSR)
    try:
        r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build(); print('built')"], cwd=tree,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=300)
    finally:
        for p in dirs:
            p.chmod(stat.S_IRWXU)
    assert r.returncode == 0 and "built" in r.stdout, r.stderr[-3000:]
    assert files() == before
