"""NAIS hidden widths up to 1024 change no interface: the library builds, exports
the symbol list it exported before and keeps its ABI version; the width check
runs before any HIP call, so it is testable here.  No GPU."""
import ctypes
import re
import subprocess

import pytest

from conftest import load_pkg

# the exported symbols as of ABI version 3, before the wide projection kernels
EXPORTED = sorted([
    "dbsde_abi_version", "dbsde_create", "dbsde_destroy", "dbsde_last_error", "dbsde_set_stream", "dbsde_param_count",
    "dbsde_param_used_mask", "dbsde_matrix_form", "dbsde_brownian_dim", "dbsde_set_corr", "dbsde_brownian",
    "dbsde_prefetch", "dbsde_prefetch_cancel", "dbsde_loss_grad", "dbsde_net_u", "dbsde_net_u_vjp", "dbsde_net_u_xvjp",
    "dbsde_net_u_jet", "dbsde_pde_residual", "dbsde_optimizer_step", "dbsde_exact", "dbsde_hjb_mc", "dbsde_mc_value",
    "dbsde_profile_enable", "dbsde_profile_count", "dbsde_profile_read", "dbsde_profile_reset", "dbsde_vec_reduce",
    "dbsde_vec_axpby", "dbsde_lbfgs_direction", "dbsde_train_step", "dbsde_stream_order_by_events",
])


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    import importlib
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def test_library_builds_with_the_same_exports(lib):
    pkg = load_pkg()
    assert sorted(pkg._lib.EXPORTED) == EXPORTED
    assert lib.dbsde_abi_version() == pkg._lib.ABI_VERSION == 3
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert sorted(set(re.findall(r"\bT (dbsde_\w+)", out))) == EXPORTED


def create(lib, pkg, mode, width, depth=4):
    cfg = pkg._lib.Config()
    layers = [9] + depth * [width] + [1]
    for k, v in enumerate(layers):
        cfg.layers[k] = v
    cfg.mode, cfg.activation, cfg.n_layers = pkg._lib.MODES[mode], 0, len(layers)
    ctx = ctypes.c_void_p()
    rc = lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx))
    msg = lib.dbsde_last_error(None).decode()
    if ctx.value:
        lib.dbsde_destroy(ctx)
    return rc, msg


@pytest.mark.parametrize("mode", ["NAIS-Net", "Naisnet"])
def test_width_check(lib, mode):
    """1025 is refused with a message naming 1024; 129 .. 1024 pass the layout
    checks (without a GPU the call then stops at the device query)."""
    pkg = load_pkg()
    rc, msg = create(lib, pkg, mode, 1025)
    assert rc == pkg._lib.DBSDE_EINVAL and "1024" in msg, (rc, msg)
    for width in (129, 144, 272, 1024):
        rc, msg = create(lib, pkg, mode, width)
        assert rc != pkg._lib.DBSDE_EINVAL, (width, rc, msg)
