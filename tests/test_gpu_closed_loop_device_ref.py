"""The closed loop with the tracker's reference taken from the device-resident map (closed_loop.run(device_reference=True):
esvo_map_cloud_build + esvo_track_set_reference_from_cloud at every re-reference) against the same loop on the host route
(download, select, upload): the same points reach the tracker, so every pose, every tick's point count and the final map are
equal as bytes."""
import numpy as np
import pytest

from esvo_amd import closed_loop

pytestmark = pytest.mark.gpu


def test_device_reference_reproduces_the_host_route():
    host = closed_loop.run(n_ticks=6, reref=3)                      # references twice after the SGM bootstrap: at ticks 1 and 4
    dev = closed_loop.run(n_ticks=6, reref=3, device_reference=True)
    assert len(host["poses"]) == len(dev["poses"]) == 6
    assert np.asarray(dev["poses"]).tobytes() == np.asarray(host["poses"]).tobytes()
    assert dev["points"] == host["points"] and min(host["points"]) > 0
    assert len(dev["map"]) == len(host["map"]) > 500
    assert dev["map"].tobytes() == host["map"].tobytes()
    assert dev["sgm_points"] == host["sgm_points"]
