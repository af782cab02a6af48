"""RegProblemLM::setProblem's point loop on the device-resident cloud (esvo_track_set_reference_from_cloud) against the host route
esvo_track_set_reference(cloud[order]) on the same handle: residuals, Jacobian, normal equations and the registration must be
equal as bytes -- the reference points are the same doubles whichever way they arrived."""
import ctypes as C

import numpy as np
import pytest

import map_cloud_cases as MC
from esvo_amd import lib

pytestmark = pytest.mark.gpu


def _evaluate(dev, n, T_ref_left):
    """everything the tracker computes from the reference, as a list of (label, bytes)"""
    R_, t_ = T_ref_left[:3, :3].copy(), T_ref_left[:3, 3].copy()
    Tw = np.linalg.inv(T_ref_left)
    out = []
    for off, cnt in ((0, 300), (300, 300), (n - 100, 300), (n, 5)):        # ... the tail batch and the batch past the end
        for huber in (True, False):
            r = dev.track_residuals(Tw, off, cnt, huber=huber, huber_threshold=50.0)
            assert len(r) == max(0, min(cnt, n - off))
            out.append((f"residuals {off} {cnt} {huber}", r.tobytes()))
    for off, cnt in ((0, 300), (600, 300), (n - 7, 300)):
        out.append((f"jacobian {off} {cnt}", np.ascontiguousarray(dev.track_jacobian(R_, t_, off, cnt)).tobytes()))
    Rs = np.stack([R_, R_, np.eye(3)])
    ts = np.stack([t_, t_ + np.array([1e-3, -2e-3, 5e-4]), np.zeros(3)])
    H, b, cost, m = dev.track_normal_equations_batch(Rs, ts, 0, n)
    assert m == n
    out.append(("normal equations x 3", H.tobytes() + b.tobytes() + cost.tobytes()))
    for on_device in (False, True):
        R, t, info, trace = dev.track_solve(n, np.eye(3), np.zeros(3), batch_size=300, on_device=on_device)
        assert info.iterations >= 1
        out.append((f"solve on_device={on_device}", R.tobytes() + t.tobytes() + C.string_at(C.addressof(info), C.sizeof(info)) + trace.tobytes()))
    return out


def _same(a, b):
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        assert x == y, k


@pytest.mark.parametrize("name", ["upenn", "dsec"])
def test_reference_from_cloud_equals_the_host_route(request, name):
    dev, p, stream, t, ts_left = MC.ticked(request, name)
    n_cloud = dev.map_cloud_build()
    cloud = dev.map_cloud()
    assert n_cloud == len(cloud) > 300
    rng = np.random.default_rng(11)
    draws = rng.integers(0, 2**31, size=2000, dtype=np.uint32)          # the rand() of the swaps, RegProblemLM.cpp:49
    order = lib.stochastic_order(n_cloud, 2000, draws)                  # (clamped to the cloud, as :39-40)
    n = len(order)
    assert n == min(2000, n_cloud) and len(set(order.tolist())) == n and not np.array_equal(order, np.arange(n))
    assert lib.stochastic_order_c(n_cloud, 2000, draws).tobytes() == order.tobytes()
    T = stream.pose(t)
    T_ref_left = np.linalg.inv(T) @ stream.pose(t + 8_000_000)
    dev.track_set_current(None, 5)
    dev.track_set_reference(cloud[order], T)
    host = _evaluate(dev, n, T_ref_left)
    dev.track_set_reference_from_cloud(order, T)
    device = _evaluate(dev, n, T_ref_left)
    _same(host, device)
    dev.track_set_reference(cloud[order], T)                            # ... and back: nothing of the device route lingers
    _same(host, _evaluate(dev, n, T_ref_left))


def test_list_order_and_repeated_indices(request):
    dev, p, stream, t, ts_left = MC.ticked(request, "upenn")
    n_cloud = dev.map_cloud_build()
    cloud = dev.map_cloud()
    T = stream.pose(t)
    T_ref_left = np.linalg.inv(T) @ stream.pose(t + 8_000_000)
    R_, t_ = T_ref_left[:3, :3].copy(), T_ref_left[:3, 3].copy()
    dev.track_set_current(None, 5)

    def sums(n):
        H, b, cost, m = dev.track_normal_equations(R_, t_, 0, n + 50)   # (the batch is clamped to the reference's size)
        assert m == n
        return H.tobytes() + b.tobytes() + np.float64(cost).tobytes() + dev.track_residuals(np.linalg.inv(T_ref_left), 0, n + 50).tobytes()

    # order=None: the first min(n, cloud) points in list order
    for n_ask, n_is in ((300, 300), (n_cloud + 1234, n_cloud)):
        dev.track_set_reference(cloud[:n_is], T)
        want = sums(n_is)
        dev.track_set_reference_from_cloud(None, T, n=n_ask)
        assert sums(n_is) == want
    # an index may repeat (the reference's swaps never produce one, a caller's own selection may)
    order = np.array([5, 5, 0, n_cloud - 1, 5, 17, 0] * 40, np.uint32)
    dev.track_set_reference(cloud[order], T)
    want = sums(len(order))
    dev.track_set_reference_from_cloud(order, T)
    assert sums(len(order)) == want
