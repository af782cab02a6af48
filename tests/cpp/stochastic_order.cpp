// stochastic_order.cpp -- tests/test_stochastic_order.py: esvo_hip::stochastic_order (include/esvo_hip.hpp, host code, no library)
// on cases read from a file.  Usage: stochastic_order <in.bin> <out.bin>; in.bin holds cases back to back, each
// [n_cloud u64 | n_take u64 | n_draws u64 | draws u32 x n_draws]; out.bin receives per case [count u64 | order u32 x count].
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <vector>

#include "esvo_hip.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::ofstream o(argv[2], std::ios::binary);
  if (!f.is_open() || !o.is_open()) return 2;
  uint64_t head[3];
  int cases = 0;
  while (f.read(reinterpret_cast<char*>(head), sizeof(head))) {
    std::vector<uint32_t> draws(head[2]);
    if (head[2] && !f.read(reinterpret_cast<char*>(draws.data()), (std::streamsize)(head[2] * sizeof(uint32_t)))) return 3;
    const uint64_t n_out = head[1] < head[0] ? head[1] : head[0];
    if (draws.size() < n_out) return 4;
    std::vector<uint32_t> order(n_out);
    const uint64_t n = esvo_hip::stochastic_order((size_t)head[0], (size_t)head[1], draws.data(), order.data());
    if (n != n_out) return 5;
    o.write(reinterpret_cast<const char*>(&n), sizeof(n));
    o.write(reinterpret_cast<const char*>(order.data()), (std::streamsize)(n * sizeof(uint32_t)));
    ++cases;
  }
  std::printf("%d cases\n", cases);
  return 0;
}
