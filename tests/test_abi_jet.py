"""dbsde_net_u_jet and dbsde_pde_residual in the C ABI: declared, exported,
bound, validating their arguments before any HIP call, and additive (the ABI
version stays 3).  No GPU."""
import importlib
import os
import re

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "dbsde.h")


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def _decl(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", txt, flags=re.M)
    assert decl, f"include/dbsde.h does not declare {name}"
    return [a.strip() for a in decl.group(1).split(",")], txt


def test_header_declares_and_binding_binds_them(lib):
    pkg = load_pkg()
    args, txt = _decl("dbsde_net_u_jet")
    assert len(args) == 9 and args[-3].endswith("V") and args[-2].endswith("d1") and args[-1].endswith("d2")
    assert "dbsde_net_u_jet" in pkg._lib.EXPORTED and len(lib.dbsde_net_u_jet.argtypes) == 9
    args, _ = _decl("dbsde_pde_residual")
    assert len(args) == 6 and "dbsde_pde_terms" in args[-1]
    assert "dbsde_pde_residual" in pkg._lib.EXPORTED and len(lib.dbsde_pde_residual.argtypes) == 6
    struct = re.search(r"typedef struct dbsde_pde_terms\s*\{([^}]*)\}", txt)
    assert struct, "include/dbsde.h does not define dbsde_pde_terms"
    names = re.findall(r"\*\s*(\w+)", struct.group(1))
    assert names == ["u", "u_t", "drift", "diffusion", "phi", "residual", "scale"]
    assert [n for n, _ in pkg._lib.PdeTerms._fields_] == names == list(pkg.NativeSolver.PDE_TERMS)


def test_null_context_is_einval(lib):
    pkg = load_pkg()
    assert lib.dbsde_net_u_jet(None, None, 1, None, None, 1, None, None, None) == pkg._lib.DBSDE_EINVAL
    assert b"NULL" in lib.dbsde_last_error(None)
    assert lib.dbsde_pde_residual(None, None, 1, None, None, None) == pkg._lib.DBSDE_EINVAL
    assert b"NULL" in lib.dbsde_last_error(None)


def test_abi_version_is_still_3(lib):
    pkg = load_pkg()
    assert lib.dbsde_abi_version() == 3 == pkg._lib.ABI_VERSION


def test_solver_methods_require_an_output():
    pkg = load_pkg()
    with pytest.raises(ValueError):
        pkg.NativeSolver.net_u_jet(object(), None, None, None, None)
    with pytest.raises(ValueError):
        pkg.NativeSolver.pde_residual(object(), None, None, None)
