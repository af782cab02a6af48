// gpc.cpp -- tests/test_gpu_gpc.py::test_cpp_layer: esvo_hip::GlobalPointCloud (include/esvo_hip.hpp) on a map fused from one
// frame.  Usage: gpc <dir> <width> <height>; reads <dir>/{params,P0,P1,lut0,lut1,mx0,mx1,my0,my1}.bin, the observation
// <dir>/{t,tsl,tsr,Tobs}.bin, a frame of DepthPoints <dir>/frame.bin with its pose table <dir>/poses.bin and the range
// <dir>/range.bin.  Writes <dir>/out.bin: [near points u64 | global points u64 | refreshed flag of the first update u64 | of a second
// update at the same stamp u64 | the near cloud | the global cloud], both as float triples.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "esvo_hip.hpp"

template <class T>
static std::vector<T> load(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) throw std::runtime_error("cannot read " + path);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string d = std::string(argv[1]) + "/";
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  try {
    auto prm = load<esvo_params_t>(d + "params.bin");
    std::vector<double> P[2] = {load<double>(d + "P0.bin"), load<double>(d + "P1.bin")};
    std::vector<float> lut[2] = {load<float>(d + "lut0.bin"), load<float>(d + "lut1.bin")};
    std::vector<float> mx[2] = {load<float>(d + "mx0.bin"), load<float>(d + "mx1.bin")};
    std::vector<float> my[2] = {load<float>(d + "my0.bin"), load<float>(d + "my1.bin")};
    esvo_calib_t cal[2];
    for (int c = 0; c < 2; ++c) {
      cal[c].width = W; cal[c].height = H;
      std::copy(P[c].begin(), P[c].begin() + 12, cal[c].P);
      cal[c].rect_lut = lut[c].data(); cal[c].rect_mask = nullptr;
      cal[c].map_x = mx[c].data(); cal[c].map_y = my[c].data();
    }
    auto ctx = std::make_shared<esvo_hip::Context>(prm.at(0), cal[0], cal[1]);
    auto tsl = load<uint8_t>(d + "tsl.bin"), tsr = load<uint8_t>(d + "tsr.bin");
    auto Tobs = load<double>(d + "Tobs.bin");
    const uint64_t t_ns = load<uint64_t>(d + "t.bin").at(0);
    const double range = load<double>(d + "range.bin").at(0);
    ctx->check(esvo_map_set_observation(ctx->handle(), t_ns, tsl.data(), tsr.data(), Tobs.data()), "esvo_map_set_observation");
    auto frame = load<esvo_hip::DepthPoint>(d + "frame.bin");
    auto poses = load<double>(d + "poses.bin");
    esvo_hip::StampTransformationMap st_map;
    for (size_t i = 0; i + 16 <= poses.size(); i += 16) st_map.emplace(t_ns, poses.data() + i);
    esvo_hip::DepthFusion fusor(ctx);
    fusor.pushFrame(frame, st_map);
    fusor.update();
    // the node's side: visualize_range, visualizeGPC_interval 1 s, NumGPC_added_per_refresh 40
    esvo_hip::GlobalPointCloud gpc(ctx, range, 1.0, 40);
    if (gpc.size() != 0) throw std::runtime_error("the global cloud is not empty after its construction");
    const uint64_t first = gpc.update(t_ns) ? 1 : 0, second = gpc.update(t_ns) ? 1 : 0;
    std::vector<float> near_xyz, global_xyz;
    gpc.nearCloud(range, near_xyz);
    gpc.get(global_xyz);
    const esvo_gpc_stats_t st = gpc.stats();
    if (st.total_points != global_xyz.size() / 3 || st.last_near != near_xyz.size() / 3 || st.updates != 2 || st.refreshes != first)
      throw std::runtime_error("the stats disagree with the clouds");
    const uint64_t head[4] = {near_xyz.size() / 3, global_xyz.size() / 3, first, second};
    std::ofstream o(d + "out.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(head), sizeof(head));
    o.write(reinterpret_cast<const char*>(near_xyz.data()), (std::streamsize)(near_xyz.size() * sizeof(float)));
    o.write(reinterpret_cast<const char*>(global_xyz.data()), (std::streamsize)(global_xyz.size() * sizeof(float)));
    std::printf("%zu near points, %zu global points\n", near_xyz.size() / 3, global_xyz.size() / 3);
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << "\n";
    return 1;
  }
  return 0;
}
