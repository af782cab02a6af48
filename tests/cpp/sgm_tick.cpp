// sgm_tick.cpp -- tests/test_gpu_sgm_tick.py::test_cpp_semi_global_matching_layer: esvo_hip::MappingAtTimeSemiGlobalMatching and
// DepthFusion::pushDisparityFrame (include/esvo_hip.hpp) on inputs dumped by the test.  Usage: sgm_tick <dir> <width> <height>
// <ticks>; reads <dir>/{params,P0,P1,lut0,lut1,mx0,mx1,my0,my1,left}.bin and per tick k <dir>/{t,tsl,tsr,Tobs,disp,sel}<k>.bin.
// Ticks 0 .. n-2 go through MappingAtTimeSemiGlobalMatching (host Time Surfaces), the last one through the seam; writes the last
// DepthMap to <dir>/map.bin and the per-tick point counts to <dir>/counts.bin.
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
  if (argc != 5) return 2;
  const std::string d = std::string(argv[1]) + "/";
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n_ticks = std::atoi(argv[4]);
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
    auto left = load<esvo_event_t>(d + "left.bin");
    esvo_hip::TimeSurface tsL(ctx, 0);
    tsL.eventsCallback(left.data(), left.size());
    esvo_hip::DepthFusion fusor(ctx);
    std::vector<uint64_t> counts;
    for (int k = 0; k < n_ticks; ++k) {
      const std::string s = std::to_string(k);
      auto tsl = load<uint8_t>(d + "tsl" + s + ".bin"), tsr = load<uint8_t>(d + "tsr" + s + ".bin");
      auto Tobs = load<double>(d + "Tobs" + s + ".bin");
      esvo_hip::StampedTimeSurfaceObs obs;
      obs.t_ns = load<uint64_t>(d + "t" + s + ".bin").at(0);
      obs.TS_left = tsl.data(); obs.TS_right = tsr.data();
      std::copy(Tobs.begin(), Tobs.begin() + 16, obs.T_world_cam);
      if (k + 1 < n_ticks) {
        counts.push_back(esvo_hip::MappingAtTimeSemiGlobalMatching(*ctx, obs));
      } else {  // the node keeps its own StereoSGBM and dataTransferring
        auto disp = load<int16_t>(d + "disp" + s + ".bin");
        auto sel = load<uint32_t>(d + "sel" + s + ".bin");
        std::vector<esvo_hip::Event> ev;
        for (uint32_t i : sel) ev.push_back(left.at(i));
        ctx->check(esvo_map_set_observation(ctx->handle(), obs.t_ns, obs.TS_left, obs.TS_right, obs.T_world_cam), "esvo_map_set_observation");
        counts.push_back(fusor.pushDisparityFrame(disp.data(), ev));
      }
    }
    std::vector<esvo_hip::DepthPoint> map;
    fusor.getDepthMap(map);
    std::ofstream o(d + "map.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(map.data()), (std::streamsize)(map.size() * sizeof(map[0])));
    std::ofstream c(d + "counts.bin", std::ios::binary);
    c.write(reinterpret_cast<const char*>(counts.data()), (std::streamsize)(counts.size() * sizeof(counts[0])));
    std::printf("%zu map elements\n", map.size());
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << "\n";
    return 1;
  }
  return 0;
}
