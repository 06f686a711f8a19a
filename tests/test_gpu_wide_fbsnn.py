"""The FBSNN class surface at state dimensions above 126 (needs an MI355X):
construction, loss_function, train, predict, device_step with a correlated
problem (dbsde_set_corr at n = 160: the wide correlated rollout), a plugin
subclass on the generic path (its network pass is native) and the reference's
jacobian(net_u) call.  Bounds as tests/test_gpu_parity.py and
tests/test_gpu_netu_xgrad.py."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from oracle import fbsnn_ref as fr

pytestmark = pytest.mark.gpu
T = 1.0


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bsb200(pkg, dev):
    """(model, oracle on its initial weights), shared; train() runs last in its test."""
    D, M, N = 200, 20, 3
    layers = [D + 1] + 4 * [48] + [1]
    torch.manual_seed(0)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), T, M, N, D, layers, "NAIS-Net", "Sine", device=dev)
    m.log_print = False
    oracle = fr.build_model("NAIS-Net", layers, "Sine")
    fr.set_flat_params(oracle, m.params.cpu().numpy())
    return m, oracle


def test_bsb_loss_function_train_predict(pkg, dev, bsb200):
    m, oracle = bsb200
    D, M, N = m.D, m.M, m.N
    t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
    Xi = torch.ones(1, D)
    ref = fr.loss_and_grads(oracle, fr.make_problem("bsb", D), t, W, Xi, M, D)
    m.model.zero_grad(set_to_none=True)
    loss, X, Y, y0 = m.loss_function(t.to(dev), W.to(dev), Xi.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss), ref["loss"], rtol=1e-4)
    np.testing.assert_array_equal(X.cpu().numpy(), ref["X"])
    np.testing.assert_allclose(Y.cpu().numpy(), ref["Y"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Y"]).max()))
    named = dict(m.model.named_parameters())
    g = torch.cat([(named[n].grad if named[n].grad is not None else torch.zeros_like(named[n])).reshape(-1)
                   for n in m.model.state_dict()]).cpu().numpy()
    used = ref["used"]
    assert np.all(g[~used] == 0)
    np.testing.assert_allclose(g[used], ref["grad"][used], rtol=0, atol=2e-4 * np.abs(ref["grad"]).max())
    # predict: [M, N+1, .]
    Xp, Yp = m.predict(np.ones((1, D)), t.numpy(), W.numpy())
    assert tuple(Xp.shape) == (M, N + 1, D) and tuple(Yp.shape) == (M, N + 1, 1)
    np.testing.assert_array_equal(Xp.cpu().numpy(), ref["X"])
    # train
    np.random.seed(1)
    graph = m.train(3, 1e-3)
    assert graph.shape[0] == 2 and len(m.training_loss) >= 1 and np.all(np.isfinite(m.training_loss))
    assert torch.all(torch.isfinite(m.params))


def test_jacobian_rows_are_Du(pkg, dev):
    """StabilityCheck's jacobian(net_u, S) call (with_corr...py:856-877) on 3 points at D = 200."""
    D, R = 200, 3
    layers = [D + 1] + 4 * [48] + [1]
    torch.manual_seed(3)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), T, 8, 3, D, layers, "NAIS-Net", "Sine", device=dev)
    rs = np.random.RandomState(1)
    tt = torch.from_numpy(rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)).to(dev)
    S = torch.from_numpy((1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)).to(dev)
    J = torch.autograd.functional.jacobian(lambda s: m.net_u(tt, s)[0], S).cpu()
    assert J.shape == (R, 1, R, D)
    with torch.no_grad():
        _, du = m.net_u(tt, S)
    du = du.cpu()
    for r in range(R):
        for q in range(R):
            if r != q:
                assert torch.all(J[r, 0, q] == 0), (r, q)
    Jd = torch.stack([J[r, 0, r] for r in range(R)])
    scale = float(du.abs().max())
    assert scale > 0
    np.testing.assert_allclose(Jd.numpy(), du.numpy(), rtol=0, atol=1e-4 * scale)


def test_correlated_basket_constructs_and_steps(pkg, dev):
    D, M, N = 160, 32, 8
    np.random.seed(2)
    m = pkg.BasketCallOption(np.ones((1, D)), T, M, N, D, 1.0, [D + 1] + 4 * [32] + [1], "Naisnet", "Tanh",
                             correlation_type="random_correlation", device=dev)
    assert m.native_coefficients and m._L is not None and m._L.shape == (D, D)
    assert np.abs(np.tril(m._L, -1)).max() > 0
    opt = m.new_optimizer_state("Adam", 1e-3)
    l1 = float(m.device_step(opt, seed=1, next_seed=2))
    l2 = float(m.device_step(opt, seed=2))
    assert np.isfinite(l1) and np.isfinite(l2)
    with pytest.raises(ValueError):             # the comparator keeps its D <= 128 limit for a Cholesky factor
        m.mc_value(np.zeros(2), np.ones((2, D)), mc=256)
    np.random.seed(3)
    out = m.train(2, 1e-3)
    assert len(out) == 4 and np.isfinite(out[1])
    assert torch.all(torch.isfinite(m.params))


def test_plugin_subclass_on_the_generic_path(pkg, dev):
    """sigma = 0.3 diag(X) differs from the inherited spec: the generic path,
    whose u / Z and network backward are native, at D = 150."""
    class MyBSB(pkg.BlackScholesBarenblatt):
        def sigma_tf(self, t, X, Y):
            return 0.3 * torch.diag_embed(X)

    D, M, N = 150, 16, 4
    torch.manual_seed(17)
    with pytest.warns(UserWarning, match="sigma_tf"):
        m = MyBSB(np.ones((1, D)), T, M, N, D, [D + 1, 16, 16, 16, 16, 1], "NAIS-Net", "Sine", device=dev)
    assert not m.native_coefficients
    np.random.seed(18)
    t, W = m.fetch_minibatch()
    before = m.params.clone()
    opt = m.new_optimizer_state("Adam", 1e-3)
    loss, _ = m.train_step(t, W, opt, "Adam", 1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    used = m.solver.used_mask.to(dev)
    assert torch.all(torch.isfinite(m.grad)) and float(m.grad[used].abs().max()) > 0
    assert float((m.params - before).abs().max()) > 0
