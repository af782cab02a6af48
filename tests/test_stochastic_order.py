"""The order RegProblemLM::setProblem's stochastic swaps leave (RegProblemLM.cpp:45-49), computed from the cloud's size and the
draws alone: esvo_amd.lib.stochastic_order and the C++ inline esvo_hip::stochastic_order (include/esvo_hip.hpp) against the
literal swaps on an explicit array.  No GPU: the library's C entry, which calls the C++ inline, is checked in
tests/test_gpu_map_cloud.py (loading the library may need the runtime)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from esvo_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def literal_swaps(n_cloud, n_take, draws):
    """for (i = 0; i < numPoints_; i++) std::swap(v[i], v[i + rand() % (v.size() - i)]) on the identity"""
    v = np.arange(n_cloud, dtype=np.uint32)
    n_take = min(n_take, n_cloud)                                     # :39-40
    for i in range(n_take):
        j = i + int(draws[i]) % (n_cloud - i)
        v[i], v[j] = v[j], v[i]
    return v[:n_take].copy()


def cases():
    out = []
    for n_cloud in (1, 2, 5, 2000, 100_003):
        for n_take in (0, 1, n_cloud, n_cloud + 7):
            rng = np.random.default_rng(1000 * n_cloud + n_take)
            draws = rng.integers(0, 2**31, size=max(n_take, 2), dtype=np.uint32)   # rand(): 0 .. RAND_MAX = 2^31 - 1
            draws[0] = 0
            draws[1::5] = 2**31 - 1
            draws[3::7] = 0
            out.append((n_cloud, n_take, draws))
    return out


@pytest.mark.parametrize("n_cloud,n_take,draws", cases(), ids=lambda v: str(v) if np.isscalar(v) else "draws")
def test_python_function_equals_the_literal_swaps(n_cloud, n_take, draws):
    got, want = lib.stochastic_order(n_cloud, n_take, draws), literal_swaps(n_cloud, n_take, draws)
    assert got.dtype == np.uint32 and len(got) == min(n_take, n_cloud)
    assert got.tobytes() == want.tobytes()
    assert len(set(got.tolist())) == len(got)                          # a partial permutation: no point taken twice


def test_cpp_inline_equals_the_literal_swaps(tmp_path):
    exe = str(tmp_path / "stochastic_order")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stochastic_order.cpp"), "-o", exe])
    cs = cases()
    with open(tmp_path / "in.bin", "wb") as f:
        for n_cloud, n_take, draws in cs:
            f.write(struct.pack("<3Q", n_cloud, n_take, len(draws)))
            f.write(draws.astype("<u4").tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    blob = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for n_cloud, n_take, draws in cs:
        (n,) = struct.unpack_from("<Q", blob, pos)
        pos += 8
        want = literal_swaps(n_cloud, n_take, draws)
        assert n == len(want)
        assert blob[pos:pos + 4 * n] == want.astype("<u4").tobytes(), (n_cloud, n_take)
        pos += 4 * n
    assert pos == len(blob)
