// ts_history.cpp -- tests/test_gpu_ts_history.py::test_cpp_layer: esvo_hip::TimeSurfaceHistory, DepthFusion::setObservationAt and
// RegProblemLM::setCurrentAt (include/esvo_hip.hpp) against the host-image route on the same handle.
// Usage: ts_history <dir> <width> <height>; reads <dir>/{params,P0,P1,lut0,lut1,mx0,mx1,my0,my1}.bin, twelve stamps <dir>/stamps.bin
// with their frames <dir>/{left,right}.bin (12 x W*H bytes each), the observation's pose <dir>/Tobs.bin, its events <dir>/ev.bin and
// pose table <dir>/{pose_stamps,poses}.bin, the tracker's inputs <dir>/{xyz,Tref,R,tr}.bin.
// Writes <dir>/out.bin: [matches of the host route u64 | of the history route u64 | chosen index u64 | H b cost (43 doubles) host
// route, newest frame | history route | host route, older frame | history route | after a refused stamp] and
// <dir>/{emp_host,emp_hist}.bin, the matches of the two routes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
template <class T>
static void save(const std::string& path, const std::vector<T>& v) {
  std::ofstream o(path, std::ios::binary);
  o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
static void expect(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(std::string("ts_history: ") + what);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string d = std::string(argv[1]) + "/";
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  const size_t npx = (size_t)W * H;
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
    auto stamps = load<uint64_t>(d + "stamps.bin");
    auto left = load<uint8_t>(d + "left.bin"), right = load<uint8_t>(d + "right.bin");
    const size_t N = stamps.size();
    expect(N == 12 && left.size() == N * npx && right.size() == N * npx, "twelve stamps with their frames");

    esvo_hip::TimeSurfaceHistory hist(ctx);
    bool refused = false;
    try { hist.stamps(); } catch (const esvo_hip::Error& e) { refused = e.code == ESVO_ERR_STATE; }
    expect(refused, "the history is off until it is configured");
    // three pairs retained out of four, then the full twelve
    hist.configure(3);
    for (size_t i = 0; i < 4; ++i) {
      hist.put(stamps[i], 0, left.data() + i * npx);
      if (i != 2) hist.put(stamps[i], 1, right.data() + i * npx);
    }
    std::vector<uint8_t> cams, img;
    expect(hist.stamps(&cams) == std::vector<uint64_t>(stamps.begin() + 1, stamps.begin() + 4), "the three newest stamps are retained");
    expect(cams == std::vector<uint8_t>({3, 1, 3}), "left-only entry");
    hist.get(stamps[3], 1, img);
    expect(std::memcmp(img.data(), right.data() + 3 * npx, npx) == 0, "get returns the frame that was put");
    hist.configure(12);
    expect(hist.stamps().empty(), "reconfiguring empties the history");
    for (size_t i = 0; i < N; ++i) {
      hist.put(stamps[i], 0, left.data() + i * npx);
      hist.put(stamps[i], 1, right.data() + i * npx);
    }
    // dataTransferring: no pose at the second newest stamp -> the one before it
    auto Tobs = load<double>(d + "Tobs.bin");
    esvo_hip::StampedTimeSurfaceObs obs;
    size_t asked = 0;
    const bool got = hist.selectObservation(false, [&](uint64_t t, double* T) {
      ++asked;
      if (t == stamps[N - 2]) return false;
      std::copy(Tobs.begin(), Tobs.begin() + 16, T);
      return true;
    }, obs);
    expect(got && obs.t_ns == stamps[N - 3] && asked == 2, "the second newest pair with a pose");
    expect(std::equal(Tobs.begin(), Tobs.begin() + 16, obs.T_world_cam), "the pose of the lookup");
    esvo_hip::StampedTimeSurfaceObs init;
    expect(hist.selectObservation(true, nullptr, init) && init.t_ns == stamps[N - 2] && init.T_world_cam[0] == 1 && init.T_world_cam[3] == 0,
           "INITIALIZATION takes the second newest with the identity");
    const size_t k = N - 3;

    // mapper: block matching on the host images of that pair against the retained pair
    auto ev = load<esvo_hip::Event>(d + "ev.bin");
    auto pose_stamps = load<uint64_t>(d + "pose_stamps.bin");
    auto poses = load<double>(d + "poses.bin");
    esvo_hip::StampTransformationMap st_map;
    for (size_t i = 0; i < pose_stamps.size(); ++i) st_map.emplace(pose_stamps[i], poses.data() + 16 * i);
    esvo_hip::StampedTimeSurfaceObs host = obs;
    host.TS_left = left.data() + k * npx;
    host.TS_right = right.data() + k * npx;
    esvo_hip::EventBM bm(ctx);
    esvo_hip::DepthFusion fusor(ctx);
    std::vector<esvo_hip::EventMatchPair> emp_host, emp_hist;
    bm.createMatchProblem(&host, &st_map, &ev);
    bm.match_all_HyperThread(emp_host);
    host.TS_left = left.data();                  // another pair in between; the events and the pose table stay
    host.TS_right = right.data();
    bm.createMatchProblem(&host, &st_map, &ev);
    fusor.setObservationAt(obs.t_ns, obs.T_world_cam);
    bm.match_all_HyperThread(emp_hist);
    save(d + "emp_host.bin", emp_host);
    save(d + "emp_hist.bin", emp_hist);

    // tracker: the newest frame and an older one
    auto xyz = load<float>(d + "xyz.bin");
    auto Tref = load<double>(d + "Tref.bin"), R = load<double>(d + "R.bin"), tr = load<double>(d + "tr.bin");
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
    for (size_t i : {N - 1, (size_t)4}) {
      prob.setProblem(xyz.data(), xyz.size() / 3, Tref.data(), left.data() + i * npx);
      sums();
      prob.setProblem(xyz.data(), xyz.size() / 3, Tref.data(), left.data() + ((i + 3) % N) * npx);   // another frame in between
      prob.setCurrentAt(stamps[i]);
      sums();
    }
    refused = false;
    try { prob.setCurrentAt(stamps[N - 1] + 1); } catch (const esvo_hip::Error& e) { refused = e.code == ESVO_ERR_STATE; }
    expect(refused, "a stamp that is not retained is refused");
    sums();   // ... and the current frame stays in place
    const uint64_t head[3] = {emp_host.size(), emp_hist.size(), k};
    std::ofstream o(d + "out.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(head), sizeof(head));
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
    std::printf("%zu / %zu matches, pair %zu\n", emp_host.size(), emp_hist.size(), k);
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << "\n";
    return 1;
  }
  return 0;
}
