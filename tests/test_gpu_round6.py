"""Round-6 cases on the HIP path (needs an MI355X): the prefetch ordering.

  * a prefetched batch no step consumes ("stale": prefetch seed X, run seed Y,
    repeat) must never be rolled out into the path buffer the running step
    reads (rollout.hip launch_deferred_on falls back to pf_stream avoiding that
    buffer): the X / Y / Z exports, loss and gradient of every step equal a
    context without prefetching, bit for bit, at the north-star shape (two
    path chunks, so the held-back rollout runs on the second stream);
  * consecutive steps on alternating streams with no ordering by the caller
    (dbsde_set_stream follows torch's current stream): the context orders the
    new stream after the old one on every switch, and a prefetched rollout
    joined into one stream is waited for by a consumer on another
    (rollout.hip wait_pending), so the steps equal the single-stream,
    unprefetched ones bit for bit;
  * dropping the prefetches (prefetch_drop, an in-place Xi change, a new
    Cholesky factor) after a rollout was held back and issued on the second
    chunk stream: the next steps equal a twin that never prefetched, bit for
    bit (rollout.hip drop_all orders the stream after every pending rollout)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu
M, N = 1024, 50


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(GOLDEN, "g2_north_star.npz"))
    return {k: z[k] for k in z.files}


def _model(pkg, dev, g):
    layers = [int(v) for v in g["layers"]]
    m = pkg.BlackScholesBarenblatt(g["Xi"], 1.0, M, N, layers[0] - 1, layers, "NAIS-Net", "Sine", device=dev)
    m.params.copy_(torch.from_numpy(g["params"]).to(dev))
    return m


def _outs(m):
    D = m.state_dim
    return dict(loss=torch.empty(1, device=m.device), X=torch.empty(M * (N + 1) * D, device=m.device),
                Y=torch.empty(M * (N + 1), device=m.device), Z=torch.empty(M * (N + 1) * D, device=m.device),
                grad=torch.empty_like(m.params))


def _run_steps(m, seeds, prefetch, streams=None):
    xi = m._device_xi(0, M)
    torch.cuda.synchronize()     # params / xi written on the default stream
    res = []
    for i, seed in enumerate(seeds):
        st = streams[i % len(streams)] if streams else torch.cuda.current_stream(m.device)
        with torch.cuda.stream(st):
            if prefetch is not None and prefetch(i) is not None:
                m.solver.prefetch(M, N, xi, seed=prefetch(i))
            o = _outs(m)
            m.solver.loss_grad(m.params, M, N, xi, seed=seed, grad=o["grad"], loss=o["loss"], X=o["X"], Y=o["Y"],
                               Z=o["Z"])
        res.append(o)            # no synchronisation between steps: the ordering is what is tested
    torch.cuda.synchronize()
    return [{k: v.cpu().clone() for k, v in o.items()} for o in res]


def _same(a, b):
    for ra, rb in zip(a, b):
        for k in ra:
            torch.testing.assert_close(ra[k], rb[k], rtol=0, atol=0, msg=k)


def test_stale_prefetch_never_overwrites_the_running_step(pkg, dev, g):
    seeds = [31, 32, 33, 34, 35]
    base = _run_steps(_model(pkg, dev, g), seeds, None)
    assert all(torch.isfinite(r["loss"]).all() for r in base)
    stale = _run_steps(_model(pkg, dev, g), seeds, lambda i: 5000 + i)
    _same(stale, base)
    # a mix: the next batch, then a stale one, then the next again
    mixed = _run_steps(_model(pkg, dev, g), seeds, lambda i: (seeds[i + 1] if i + 1 < len(seeds) else None)
                       if i % 2 == 0 else 7000 + i)
    _same(mixed, base)


def test_prefetch_consumed_on_another_stream(pkg, dev, g):
    seeds = [41, 42, 43, 44, 45, 46]
    base = _run_steps(_model(pkg, dev, g), seeds, None)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    swapped = _run_steps(_model(pkg, dev, g), seeds, lambda i: seeds[i + 1] if i + 1 < len(seeds) else None,
                         streams=[s1, s2])
    _same(swapped, base)


@pytest.mark.parametrize("Mr,Nr,D", [(1024, 50, 100), (37, 13, 100), (5, 3, 7)])
def test_two_pass_rollout_equals_single_pass(pkg, dev, monkeypatch, Mr, Nr, D):
    """The in-step device rollout in two passes (rollout_draw_kernel +
    rollout_chain_kernel, paths.hpp) against rollout4_kernel
    (DBSDE_ROLLOUT2=0, read at context creation): X, Y, Z, loss and gradient
    bit for bit, also at ragged M and at N not a multiple of the 4-step Philox
    block or the 8-step load-ahead."""
    layers = [D + 1, 16, 16, 16, 16, 1]
    xi = np.random.RandomState(3).uniform(0.5, 1.5, (1, D)).astype(np.float32)

    def run(flag):
        if flag is None:
            monkeypatch.delenv("DBSDE_ROLLOUT2", raising=False)
        else:
            monkeypatch.setenv("DBSDE_ROLLOUT2", flag)
        torch.manual_seed(4)
        m = pkg.BlackScholesBarenblatt(xi, 1.0, Mr, Nr, D, layers, "NAIS-Net", "Sine", device=dev)
        o = dict(loss=torch.empty(1, device=dev), X=torch.empty(Mr * (Nr + 1) * D, device=dev),
                 Y=torch.empty(Mr * (Nr + 1), device=dev), Z=torch.empty(Mr * (Nr + 1) * D, device=dev),
                 grad=torch.empty_like(m.params))
        m.solver.loss_grad(m.params, Mr, Nr, m._device_xi(0, Mr), seed=77, grad=o["grad"], loss=o["loss"], X=o["X"],
                           Y=o["Y"], Z=o["Z"])
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}

    two, one = run(None), run("0")
    assert torch.isfinite(two["X"]).all()
    for k in two:
        torch.testing.assert_close(two[k], one[k], rtol=0, atol=0, msg=k)


def test_large_batch_is_the_sum_of_its_halves(pkg, dev, g):
    """M = 16384 paths per GPU (16x the north star: R = 835,584 rows, 13,056
    phase workgroups per launch, the two-chunk pipeline with prefetch-free
    in-step rollouts) against its two halves, drawn with the device Philox
    keyed by the global path index (path0 = 0 and 8192): X bit for bit, the
    loss and the gradient as sums over the paths (DeepBSDE.py:231-241)."""
    Ml, Nl = 16384, 50
    m = _model(pkg, dev, g)
    D = m.state_dim
    xi = m._device_xi(0, M)

    def run(M, path0):
        o = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (Nl + 1) * D, device=dev),
                 Y=torch.empty(M * (Nl + 1), device=dev), grad=torch.empty_like(m.params))
        m.solver.loss_grad(m.params, M, Nl, xi, seed=99, path0=path0, grad=o["grad"], loss=o["loss"], X=o["X"],
                           Y=o["Y"])
        torch.cuda.synchronize()
        return {k: v.cpu().double() for k, v in o.items()}

    full = run(Ml, 0)
    a, b = run(Ml // 2, 0), run(Ml // 2, Ml // 2)
    assert torch.isfinite(full["loss"]).all() and torch.isfinite(full["grad"]).all()
    torch.testing.assert_close(full["X"], torch.cat([a["X"], b["X"]]), rtol=0, atol=0)
    torch.testing.assert_close(full["Y"], torch.cat([a["Y"], b["Y"]]), rtol=0, atol=1e-5 * float(full["Y"].abs().max()))
    assert float(full["loss"]) == pytest.approx(float(a["loss"] + b["loss"]), rel=1e-5)
    g2 = a["grad"] + b["grad"]
    torch.testing.assert_close(full["grad"], g2, rtol=0, atol=2e-5 * float(g2.abs().max()))


# ---- dropping prefetches after a held-back rollout went to the second chunk stream
def _two_chunk_model(pkg, dev, monkeypatch, Xi, Ms, Ns, layers, params=None):
    """A NAIS-Net / Sine model whose context takes DBSDE_CHUNKS=2 at creation."""
    with monkeypatch.context() as mp:
        mp.setenv("DBSDE_CHUNKS", "2")
        torch.manual_seed(6)
        m = pkg.BlackScholesBarenblatt(Xi, 1.0, Ms, Ns, layers[0] - 1, layers, "NAIS-Net", "Sine", device=dev)
    if params is not None:
        m.params.copy_(torch.from_numpy(params).to(dev))
    return m


def _steps_with_a_drop(m, prefetch, between, seed2):
    """device_step(seed=1[, next_seed=2]); between(m); device_step(seed=seed2):
    the second loss and the final parameters."""
    opt = m.new_optimizer_state("Adam", 1e-3)
    m.device_step(opt, 1e-3, seed=1, next_seed=2 if prefetch else None)
    between(m)               # no synchronisation: the ordering is what is tested
    loss = m.device_step(opt, 1e-3, seed=seed2).clone()
    torch.cuda.synchronize()
    return loss.cpu(), m.params.detach().cpu().clone()


@pytest.mark.parametrize("how", ["prefetch_drop", "xi_in_place"])
def test_drop_after_a_held_back_rollout(pkg, dev, g, monkeypatch, how):
    """North-star layers and parameters at M = 256, N = 5 with DBSDE_CHUNKS=2:
    the step is the piped two-chunk one, so the prefetch of seed 2 is held back
    and rolled out on the second chunk stream (pipe2) after the join, where
    nothing orders the caller's stream after it.  Dropping it (prefetch_drop,
    or the in-place Xi change that makes device_step drop it) must leave the
    next step, whose in-step rollout may take that buffer and whose Xi copy
    is rewritten, equal to a twin that never prefetched: loss and parameters
    bit for bit.

    That the held-back rollout goes to pipe2 here, from loss_grad_impl's
    conditions (step.hip): R = Rp = 256 * 6 = 1536; the layout is the
    wave-tile one (NAIS, Wp = Dp = 112, K = 3), the step is unprofiled and
    has a gradient; the phase variant has 16, 64 or 128 rows per workgroup,
    256 paths are 16, 4 or 2 such units, an even count, so nch = 2 stays; the
    chunk boundary is row (256 / 2) * 6 = 768 whichever the variant; with
    S = 128 slices over n32 = 1536 / 32 = 48 row steps, slice k starts at row
    32 * floor(48 k / 128), which is 768 first at k = 64, a multiple of 8: so
    tnw_piped holds and launch_deferred_on(pipe2) runs, with the other path
    buffer free (first step)."""
    layers = [int(v) for v in g["layers"]]

    def between(m):
        if how == "prefetch_drop":
            m.solver.prefetch_drop()
        else:
            m.Xi.mul_(1.5)

    runs = [_steps_with_a_drop(_two_chunk_model(pkg, dev, monkeypatch, g["Xi"], 256, 5, layers, g["params"]),
                               prefetch, between, 3) for prefetch in (True, False)]
    assert torch.isfinite(runs[1][0]).all() and torch.isfinite(runs[1][1]).all()
    torch.testing.assert_close(runs[0][0], runs[1][0], rtol=0, atol=0)
    torch.testing.assert_close(runs[0][1], runs[1][1], rtol=0, atol=0)


@pytest.mark.parametrize("seed2", [2, 3])
def test_set_corr_after_a_held_back_correlated_rollout(pkg, dev, monkeypatch, seed2):
    """The same with Cholesky-correlated increments (dbsde_set_corr) and a new
    factor between the steps: the held-back rollout of seed 2 read the old
    factor, so it is dropped (seed2 = 2: the step must not consume it) and
    waited for before the factor's memory is rewritten (seed2 = 3: nor may its
    buffer be reused while it runs).

    The smallest two-chunk piped shape: the wave-tile weight gradient needs a
    NAIS net with Wp == Dp, whose smallest fused variant is width 16 (D <= 14;
    D = 2 is the smallest with a correlation to speak of), 64 rows per
    workgroup and no column-split form; two chunks of whole 64-path units
    need M = 128.  At N = 5, Rp = 768, the chunk boundary is row 384 and slice
    64 of 128 starts at row 32 * floor(24 * 64 / 128) = 384."""
    D, Ms, Ns = 2, 128, 5
    layers = [D + 1, 16, 16, 16, 16, 1]
    Xi = np.array([[1.0, 0.5]], dtype=np.float32)
    L1 = np.linalg.cholesky(np.array([[1.0, 0.5], [0.5, 1.0]]))
    L2 = np.linalg.cholesky(np.array([[1.0, -0.3], [-0.3, 1.0]]))

    def run(prefetch):
        m = _two_chunk_model(pkg, dev, monkeypatch, Xi, Ms, Ns, layers)
        m.solver.set_corr(L1)
        return _steps_with_a_drop(m, prefetch, lambda mm: mm.solver.set_corr(L2), seed2)

    with_pf, twin = run(True), run(False)
    assert torch.isfinite(twin[0]).all() and torch.isfinite(twin[1]).all()
    torch.testing.assert_close(with_pf[0], twin[0], rtol=0, atol=0)
    torch.testing.assert_close(with_pf[1], twin[1], rtol=0, atol=0)
