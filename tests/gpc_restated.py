"""publishPointCloud's global-cloud branch (esvo_Mapping.cpp:955-977) restated in a few lines over a near cloud and a voxel
filter that are handed in -- by default oracle.voxel_filter, and the near cloud of whatever mapper the caller reads (the oracle
mapper's get_pointcloud_near, or a device handle's host read-out):

    if (t.toSec() - t_last_pub_pc_ > visualizeGPC_interval_) {            // :958, a strict >
      sor.setInputCloud(pc_near_); sor.setLeafSize(leaf); sor.filter(*pc_filtered);
      numAddedPC = min(pc_filtered->size(), numAddedPC_threshold_) - 1;   // :969, size_t
      pc_global_->insert(end, pc_filtered->end() - numAddedPC, pc_filtered->end());
      t_last_pub_pc_ = t.toSec();
    }

t_last_pub_pc_ starts at 0.0 (:152); esvo_Mapping::reset clears pc_global_ (:780) and leaves t_last_pub_pc_ alone.
Where the reference is undefined the library's definitions are restated: an empty filtered cloud adds nothing (the size_t
subtraction would wrap) and still counts as a refresh; an append beyond the capacity raises and changes nothing."""
import numpy as np

from esvo_amd import rostime


def due(now, t_last_pub, interval_s):
    return now - t_last_pub > interval_s


def tail_count(n_filtered, num_added_per_refresh):
    """how many of the filtered cloud's last points are appended"""
    assert num_added_per_refresh >= 1
    return min(int(n_filtered), int(num_added_per_refresh)) - 1 if n_filtered else 0


class CapacityError(RuntimeError):
    pass


class Gpc:
    def __init__(self, visualize_range, interval_s, num_added_per_refresh, leaf=0.3, capacity_points=5_000_000, voxel_filter=None):
        if voxel_filter is None:
            from oracle import oracle as O
            voxel_filter = O.voxel_filter
        self.voxel_filter = voxel_filter
        self.visualize_range, self.interval_s, self.thr, self.leaf = float(visualize_range), float(interval_s), int(num_added_per_refresh), leaf
        self.capacity = int(capacity_points)
        self.cloud = np.zeros((0, 3), np.float32)
        self.t_last_pub = 0.0
        self.updates = self.refreshes = 0
        self.last_near = self.last_voxels = self.last_added = self.last_refreshed = 0

    def update(self, t_ns, near_cloud):
        """near_cloud: visualize_range -> (n, 3) float32, pc_near_ of the current map.  Returns the refreshed flag."""
        now = rostime.ns_to_sec(t_ns)
        if not due(now, self.t_last_pub, self.interval_s):
            self.updates += 1
            self.last_refreshed = 0
            return False
        near = np.ascontiguousarray(near_cloud(self.visualize_range), np.float32).reshape(-1, 3)
        filtered = self.voxel_filter(near, self.leaf) if len(near) else np.zeros((0, 3), np.float32)
        k = tail_count(len(filtered), self.thr)
        if len(self.cloud) + k > self.capacity:
            raise CapacityError()
        self.cloud = np.concatenate([self.cloud, filtered[len(filtered) - k:]]) if k else self.cloud
        self.t_last_pub = now
        self.updates += 1
        self.refreshes += 1
        self.last_near, self.last_voxels, self.last_added, self.last_refreshed = len(near), len(filtered), k, 1
        return True

    def reset(self):
        self.cloud = np.zeros((0, 3), np.float32)

    def counts(self):
        return (self.updates, self.refreshes, len(self.cloud), self.last_near, self.last_voxels, self.last_added, self.last_refreshed,
                self.t_last_pub)


def voxel_filter_reversed(xyz, leaf, voxel_filter=None):
    """the filter with the points of every voxel summed in REVERSED input order: the stable sort keeps equal keys in input order,
    so reversing the input reverses every voxel's chain and leaves the voxels' order alone.  What a test compares with to show
    that its cloud's bytes depend on the order of the sum."""
    if voxel_filter is None:
        from oracle import oracle as O
        voxel_filter = O.voxel_filter
    return voxel_filter(np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3)[::-1]), leaf)
