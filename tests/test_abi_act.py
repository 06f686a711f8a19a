"""SiLU and Softplus at the C boundary: DBSDE_ACT_SILU / DBSDE_ACT_SOFTPLUS
(3, 4) ride on dbsde_config.activation; the header values equal the binding's
table, the three old values keep theirs, the ABI stays version 3 with its 32
exports, activation 5 and -1 are refused, and 3 and 4 pass the argument
checks.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "dbsde.h")
ACTS = {"Sine": ("DBSDE_ACT_SINE", 0), "ReLU": ("DBSDE_ACT_RELU", 1), "Tanh": ("DBSDE_ACT_TANH", 2),
        "SiLU": ("DBSDE_ACT_SILU", 3), "Softplus": ("DBSDE_ACT_SOFTPLUS", 4)}


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def header_text():
    return open(HEADER).read()


def header_values():
    return {n: int(v) for n, v in re.findall(r"^#define (DBSDE_\w+) (-?\d+)\b", header_text(), flags=re.M)}


def header_functions():
    return sorted(set(re.findall(r"\b(dbsde_\w+)\s*\(", header_text())))


def config(pkg, activation):
    cfg = pkg._lib.Config()
    cfg.mode, cfg.activation, cfg.n_layers = 1, activation, 4
    for k, v in enumerate([5, 16, 16, 1]):
        cfg.layers[k] = v
    cfg.problem = pkg.ProblemSpec().to_c()
    return cfg


def test_header_values_equal_the_binding_table():
    pkg = load_pkg()
    hv = header_values()
    assert pkg._lib.ACTIVATIONS == {name: value for name, (_, value) in ACTS.items()}
    for name, (macro, value) in ACTS.items():
        assert hv[macro] == value, name
    assert sorted(n for n in hv if n.startswith("DBSDE_ACT_")) == sorted(m for m, _ in ACTS.values())
    # the three old values keep theirs
    assert [pkg._lib.ACTIVATIONS[n] for n in ("Sine", "ReLU", "Tanh")] == [0, 1, 2]
    nets = importlib.import_module(pkg.__name__ + ".networks")
    assert type(nets.activation_module("SiLU")) is torch.nn.SiLU
    sp = nets.activation_module("Softplus")
    assert type(sp) is torch.nn.Softplus and sp.beta == 1


def test_abi_version_and_exports_are_unchanged(lib):
    pkg = load_pkg()
    assert header_values()["DBSDE_ABI_VERSION"] == pkg._lib.ABI_VERSION == lib.dbsde_abi_version() == 3
    assert len(pkg._lib.EXPORTED) == 32 and sorted(pkg._lib.EXPORTED) == header_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert sorted(set(re.findall(r"\bT (dbsde_\w+)", out))) == sorted(pkg._lib.EXPORTED)


def test_unknown_activations_are_refused(lib):
    """Refused before any HIP call, with the context left NULL."""
    pkg = load_pkg()
    for bad in (5, -1, 6, 1 << 20):
        ctx = ctypes.c_void_p()
        cfg = config(pkg, bad)
        assert lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx)) == pkg._lib.DBSDE_EINVAL and not ctx.value, bad
        assert b"unknown activation" in lib.dbsde_last_error(None), bad


def test_the_new_values_pass_the_argument_checks(lib):
    """dbsde_create no longer refuses 3 and 4.  Without a device it stops at
    the first HIP call (not DBSDE_EINVAL, no context); with one it succeeds."""
    pkg = load_pkg()
    gpu = torch.cuda.is_available()
    for name in ("Tanh", "SiLU", "Softplus"):
        ctx = ctypes.c_void_p()
        cfg = config(pkg, ACTS[name][1])
        rc = lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx))
        err = lib.dbsde_last_error(None)
        assert rc != pkg._lib.DBSDE_EINVAL and (rc == pkg._lib.DBSDE_OK) == gpu, (name, rc, err)
        assert b"unknown activation" not in err, name
        if ctx.value:
            lib.dbsde_destroy(ctx)


def test_native_solver_names_the_five():
    pkg = load_pkg()
    with pytest.raises(ValueError) as e:
        pkg.NativeSolver("FC", [5, 16, 16, 1], "GELU", pkg.ProblemSpec(), 1.0, "cpu")
    for name in ACTS:
        assert name in str(e.value), (name, str(e.value))
    nets = importlib.import_module(pkg.__name__ + ".networks")
    with pytest.raises(ValueError) as e:
        nets.activation_module("GELU")
    for name in ACTS:
        assert name in str(e.value), (name, str(e.value))
