"""dbsde_net_u_xvjp in the C ABI: declared, exported, bound, validating its
arguments before any HIP call, and additive (the ABI version stays 3).  No GPU."""
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


def test_header_declares_and_binding_binds_it(lib):
    pkg = load_pkg()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"^int\s+dbsde_net_u_xvjp\s*\(([^)]*)\)\s*;", txt, flags=re.M)
    assert decl, "include/dbsde.h does not declare dbsde_net_u_xvjp"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 9 and args[-2].endswith("grad") and args[-1].endswith("xbar")
    assert "dbsde_net_u_xvjp" in pkg._lib.EXPORTED
    f = lib.dbsde_net_u_xvjp
    assert len(f.argtypes) == 9
    # dbsde_net_u_vjp keeps its signature
    assert re.search(r"^int\s+dbsde_net_u_vjp\s*\(", txt, flags=re.M) and len(lib.dbsde_net_u_vjp.argtypes) == 8


def test_null_context_is_einval(lib):
    pkg = load_pkg()
    assert lib.dbsde_net_u_xvjp(None, None, 1, None, None, None, None, None, None) == pkg._lib.DBSDE_EINVAL
    assert b"NULL" in lib.dbsde_last_error(None)


def test_abi_version_is_still_3(lib):
    pkg = load_pkg()
    assert lib.dbsde_abi_version() == 3 == pkg._lib.ABI_VERSION


def test_solver_method_requires_an_output():
    pkg = load_pkg()
    with pytest.raises(ValueError):
        pkg.NativeSolver.net_u_xvjp(object(), None, None, None, None, None)
