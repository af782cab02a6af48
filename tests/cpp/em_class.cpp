// em_class.cpp -- tests/test_gpu_em.py::test_cpp_event_matcher_class: esvo_hip::EventMatcher (include/esvo_hip.hpp) on inputs
// dumped by the test.  Usage: em_class <dir> <width> <height>; reads <dir>/{params,em,P0,P1,lut0,lut1,mx0,mx1,my0,my1,
// tsl,tsr,Tobs,left,right,begin,count,T}.bin, writes the matches to <dir>/out.bin.
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
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (!f.good() && !f.eof()) throw std::runtime_error("cannot read " + path);
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
    auto em = load<esvo_em_params_t>(d + "em.bin");
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
    esvo_hip::StampedTimeSurfaceObs obs;
    obs.t_ns = 1; obs.TS_left = tsl.data(); obs.TS_right = tsr.data();
    std::copy(Tobs.begin(), Tobs.begin() + 16, obs.T_world_cam);
    auto left = load<esvo_event_t>(d + "left.bin"), right = load<esvo_event_t>(d + "right.bin");
    auto begin = load<uint32_t>(d + "begin.bin"), count = load<uint32_t>(d + "count.bin");
    auto T = load<double>(d + "T.bin");
    std::vector<esvo_hip::EventSlice> slices(begin.size());
    for (size_t s = 0; s < slices.size(); ++s) {
      slices[s].begin = begin[s]; slices[s].numEvents = count[s];
      std::copy(T.begin() + 16 * s, T.begin() + 16 * s + 16, slices[s].transf);
    }
    const esvo_em_params_t& e = em.at(0);
    esvo_hip::EventMatcher matcher(ctx, e.time_threshold, e.epipolar_threshold, e.ncc_threshold,
                                   (size_t)e.patch_intensity_threshold, e.patch_valid_ratio);
    matcher.createMatchProblem(&obs, &slices, &left, &right);
    std::vector<esvo_hip::EventMatchPair> vEMP;
    matcher.match_all_HyperThread(vEMP);
    std::ofstream o(d + "out.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(vEMP.data()), (std::streamsize)(vEMP.size() * sizeof(vEMP[0])));
    std::printf("%zu matches\n", vEMP.size());
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << "\n";
    return 1;
  }
  return 0;
}
