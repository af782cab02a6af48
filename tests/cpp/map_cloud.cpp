// map_cloud.cpp -- tests/test_gpu_map_cloud.py::test_cpp_layer: DepthFusion::buildPointCloud + RegProblemLM::setProblemFromMap
// (include/esvo_hip.hpp) against getPointCloud + setProblem on the same handle.  Usage: map_cloud <dir> <width> <height>; reads
// <dir>/{params,P0,P1,lut0,lut1,mx0,mx1,my0,my1}.bin, the observation <dir>/{t,tsl,tsr,Tobs}.bin, a frame of DepthPoints
// <dir>/frame.bin with its pose table <dir>/poses.bin, the tracker's inputs <dir>/{Tref,R,tr}.bin and the draws <dir>/draws.bin.
// Writes <dir>/out.bin: [cloud points u64 | reference points u64 | H b cost (43 doubles) of the host route | the same of the device
// route | H b cost of the host route without swaps | the same of the device route].
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
    ctx->check(esvo_map_set_observation(ctx->handle(), t_ns, tsl.data(), tsr.data(), Tobs.data()), "esvo_map_set_observation");
    // the mapper's side: one frame into the window, fused into a DepthMap
    auto frame = load<esvo_hip::DepthPoint>(d + "frame.bin");
    auto poses = load<double>(d + "poses.bin");
    esvo_hip::StampTransformationMap st_map;
    for (size_t i = 0; i + 16 <= poses.size(); i += 16) st_map.emplace(t_ns, poses.data() + i);
    esvo_hip::DepthFusion fusor(ctx);
    fusor.pushFrame(frame, st_map);
    fusor.update();
    // the tracker's side
    auto Tref = load<double>(d + "Tref.bin"), R = load<double>(d + "R.bin"), tr = load<double>(d + "tr.bin");
    auto draws = load<uint32_t>(d + "draws.bin");
    esvo_hip::RegProblemConfig cfg;
    esvo_hip::RegProblemLM prob(ctx, cfg);
    std::vector<double> out;
    auto sums = [&]() {
      double Hm[36], b[6], cost = 0;
      const size_t n = prob.normalEquations(R.data(), tr.data(), Hm, b, &cost);
      if (n != prob.numPoints_) throw std::runtime_error("normal equations over fewer points than the reference holds");
      out.insert(out.end(), Hm, Hm + 36);
      out.insert(out.end(), b, b + 6);
      out.push_back(cost);
    };
    // host route: the cloud comes down, the swaps of RegProblemLM.cpp:45-49 run on it, 2000 points go up again
    std::vector<float> xyz;
    fusor.getPointCloud(xyz);
    const size_t n_cloud = xyz.size() / 3;
    const size_t n_ref = std::min(n_cloud, cfg.MAX_REGISTRATION_POINTS);
    if (draws.size() < n_ref) throw std::runtime_error("too few draws");
    std::vector<float> plain(xyz);
    for (size_t i = 0; i < n_ref; ++i) {
      const size_t j = i + (size_t)draws[i] % (n_cloud - i);
      for (int c = 0; c < 3; ++c) std::swap(xyz[3 * i + c], xyz[3 * j + c]);
    }
    prob.setProblem(xyz.data(), n_cloud, Tref.data(), tsl.data());
    sums();
    // device route: the cloud stays where the map is
    if (fusor.buildPointCloud() != n_cloud) throw std::runtime_error("buildPointCloud and getPointCloud disagree on the count");
    prob.setProblemFromMap(draws.data(), draws.size(), Tref.data(), cfg.MAX_REGISTRATION_POINTS, tsl.data());
    if (prob.numPoints_ != n_ref) throw std::runtime_error("setProblemFromMap took another number of points");
    sums();
    // ... and without swaps
    prob.setProblem(plain.data(), n_cloud, Tref.data(), tsl.data());
    sums();
    prob.setProblemFromMap(nullptr, 0, Tref.data(), cfg.MAX_REGISTRATION_POINTS, tsl.data());
    sums();
    std::vector<float> snap;
    fusor.getDevicePointCloud(snap);
    if (snap != plain) throw std::runtime_error("the device-resident cloud differs from getPointCloud");
    const uint64_t head[2] = {n_cloud, n_ref};
    std::ofstream o(d + "out.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(head), sizeof(head));
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
    std::printf("%zu cloud points, %zu reference points\n", n_cloud, n_ref);
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << "\n";
    return 1;
  }
  return 0;
}
