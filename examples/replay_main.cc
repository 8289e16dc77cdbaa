// replay_main.cc -- the sequential stereo-inertial replay WITHOUT Python: a C++ host that plays the part of the
// reference's Tracking / LocalMapping threads around the C-ABI of include/vieo_hot.h.
//
//   per frame     vieo_track_frame                 (Frame::Frame + TrackWithIMU + TrackLocalMapWithIMU, one call)
//   per key frame vieo_imu_preintegrate_batch      (the key-frame pair's pre-integration, LocalMapping side)
//                 vieo_local_bundle_adjustment_vio (Optimizer::LocalBundleAdjustmentNavStatePRV)
//                 vieo_update_normal_and_depth_batch (MapPoint::UpdateNormalAndDepth after the write-back)
//
// It is the C++ twin of vieo_slam_amd/replay.py (class Replay / tracker.TrackerReplay), same simplifications: a key
// frame every `kf_every` frames, new points only from stereo depth (CreateNewKeyFrame, src/Tracking.cc:2180-2250),
// local map = the points of the last `n_local_kfs` key frames, first frame initialised with the true state.  The map
// (key frames, points, observations) lives here on the host, as it lives in Map / KeyFrame / MapPoint in the reference.
//
//   tools/write_sequence.py seq.vseq --frames 100      # the rendered sequence, once
//   ./examples/replay_main seq.vseq [traj.bin] [--frames N] [--warmup M] [--quiet]
// --warmup M: M frames are replayed once before the timed run (code objects loaded, scratch buffers allocated).
// Prints one JSON line: frames, ms per frame (whole loop / tracking call / its GPU part), local BAs, error against the
// sequence's true trajectory; traj.bin receives the optimised vieo_navstate of every frame (176 B each).
// Built by __graft_entry__.build().
#include "replay_common.hpp"

using namespace vieo_replay;

namespace {

struct Replay : TrackerReplay {
  double ms_prep = 0, ms_post = 0, ms_finish = 0;  // the caller's own work per frame: before / after the call, bookkeeping

  explicit Replay(const Sequence& s) : TrackerReplay(s) {
    create_extractors();  // (the first frame goes through the stage entries: make_frame0)
    create_rectified_tracker(NFEAT);
  }

  // one frame: Tracking::Track for the stereo-inertial steady state
  void step(int k) {
    const auto t0 = std::chrono::steady_clock::now();
    const Frame& L = *last;
    const Frame& ref = map_updated ? *kfs.back() : L;
    const double t = S.time(k);
    vieo_track_input in;
    std::memset(&in, 0, sizeof(in));
    set_images(in, k, false), in.stride = S.W;
    run_ahead(in, k);
    int i0, ni;
    S.imu_between(ref.t, t, &i0, &ni);
    in.imu = S.imu.data() + i0, in.n_imu = ni;
    in.t_ref = ref.t, in.t_cur = t;
    in.nav_ref = ref.nav, in.nav_last = L.nav;
    if (!map_updated && L.has_prior) in.nav_prior = &L.prior_nav, in.H_prior = L.H_prior;
    last_frame_and_local_map(in);
    vieo_track_output out;
    const auto t1 = std::chrono::steady_clock::now();
    CHECK(vieo_track_frame(trk, &in, &out));
    const auto t2 = std::chrono::steady_clock::now();
    if (out.status != VIEO_TRACK_OK) {
      std::fprintf(stderr, "frame %d: IMU pre-integration failed (%d)\n", k, out.preint_status);
      std::exit(1);
    }
    const FramePtr f = adopt(k, out);
    const auto t3 = std::chrono::steady_clock::now();
    ms_frames += std::chrono::duration<double, std::milli>(t3 - t0).count();
    finish_frame(k, f);
    ms_prep += std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_post += std::chrono::duration<double, std::milli>(t3 - t2).count();
    ms_finish += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t3).count();
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s seq.vseq [traj.bin] [--frames N] [--warmup M] [--lba-lag L] [--prefetch 0|1] [--trackers T] [--quiet]\n", argv[0]);
    return 2;
  }
  const char* traj_path = nullptr;
  int n_frames = -1, warmup = 0, lba_lag = 0, n_trackers = 1, kf_every = 10, prefetch = 0;
  bool quiet = false;
  for (int i = 2; i < argc; i++) {
    if (!std::strcmp(argv[i], "--frames") && i + 1 < argc)
      n_frames = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--trackers") && i + 1 < argc)
      n_trackers = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--prefetch") && i + 1 < argc)
      prefetch = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--kf-every") && i + 1 < argc)  // (experiments: a huge value = no key frames, no local BA)
      kf_every = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--warmup") && i + 1 < argc)
      warmup = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--lba-lag") && i + 1 < argc)
      lba_lag = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--quiet"))
      quiet = true;
    else
      traj_path = argv[i];
  }
  if (!vieo_device_available()) {
    std::fprintf(stderr, "no gfx950 device: %s (there is no CPU fallback)\n", vieo_last_error());
    return 2;
  }
  Sequence S;
  if (!load_sequence(argv[1], S)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const int n = n_frames > 0 ? std::min(n_frames, S.n_frames) : S.n_frames;
  if (warmup > 1) {
    Replay Wm(S);
    Wm.lba_lag = lba_lag, Wm.prefetch = prefetch != 0, Wm.last_frame = std::min(warmup, S.n_frames) - 1;
    warm_up(Wm, warmup);
  }
  if (n_trackers > 1) {
    // N independent sequences on ONE GPU (BASELINE configs[3] "8 sequences": what a GPU of that run serves when it gets
    // more than one): every tracker has its own host thread, streams, map and LocalMapping thread; all replay the same
    // file, so every trajectory must equal the first one's bit for bit.
    std::vector<std::unique_ptr<Replay>> Rs;
    for (int i = 0; i < n_trackers; i++) {
      Rs.emplace_back(new Replay(S));
      Rs.back()->lba_lag = lba_lag, Rs.back()->kf_every = kf_every, Rs.back()->prefetch = prefetch != 0, Rs.back()->last_frame = n - 1;
      Rs.back()->initialise();
    }
    std::mutex m;
    std::condition_variable cv;
    int ready = 0;
    bool go = false;
    std::vector<double> wall(n_trackers, 0.0);
    std::vector<std::thread> th;
    for (int i = 0; i < n_trackers; i++)
      th.emplace_back([&, i] {
        {
          std::unique_lock<std::mutex> g(m);
          ready++;
          cv.notify_all();
          cv.wait(g, [&] { return go; });
        }
        const auto t0 = std::chrono::steady_clock::now();
        Replay& R = *Rs[i];
        for (int k = 1; k < n; k++) {
          const auto tk = std::chrono::steady_clock::now();
          R.before_frame(k);
          R.step(k);
          R.frame_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk).count());
        }
        wall[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        R.before_frame(1 << 30);
      });
    std::chrono::steady_clock::time_point t0;
    {
      std::unique_lock<std::mutex> g(m);
      cv.wait(g, [&] { return ready == n_trackers; });
      go = true;
      t0 = std::chrono::steady_clock::now();
    }
    cv.notify_all();
    for (auto& t : th) t.join();
    const double ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bool same = true;
    for (int i = 1; i < n_trackers; i++)
      same = same && Rs[i]->traj.size() == Rs[0]->traj.size() &&
             !std::memcmp(Rs[i]->traj.data(), Rs[0]->traj.data(), Rs[0]->traj.size() * sizeof(vieo_navstate));
    std::vector<double> all;
    double gpu = 0, call = 0;
    for (auto& R : Rs) all.insert(all.end(), R->frame_ms.begin(), R->frame_ms.end()), gpu += R->ms_gpu, call += R->ms_track;
    std::sort(all.begin(), all.end());
    const double nf = (double)(n - 1);
    double mean = 0;
    for (double v : all) mean += v;
    std::printf("{\"trackers\": %d, \"frames_per_tracker\": %d, \"frames_per_s_all_trackers\": %.2f, \"ms_per_frame_latency_mean\": %.4f, "
                "\"ms_per_frame_latency_median\": %.4f, \"ms_per_frame_latency_p99\": %.4f, \"ms_track_call_mean\": %.4f, "
                "\"ms_track_gpu_mean\": %.4f, \"slowest_tracker_ms_per_frame\": %.4f, \"identical_trajectories\": %s, \"lba_lag\": %d}\n",
                n_trackers, n - 1, 1e3 * n_trackers * nf / ms_total, mean / all.size(), all[all.size() / 2],
                all[std::min(all.size() - 1, (size_t)(0.99 * all.size()))], call / (n_trackers * nf), gpu / (n_trackers * nf),
                *std::max_element(wall.begin(), wall.end()) / nf, same ? "true" : "false", lba_lag);
    write_traj(traj_path, Rs[0]->traj);
    return same ? 0 : 1;
  }
  Replay R(S);
  R.lba_lag = lba_lag, R.kf_every = kf_every, R.prefetch = prefetch != 0, R.last_frame = n - 1;
  const RunTime rt = timed_run(R, n, quiet);
  const TruthError err = error_vs_truth(S, R.traj, n);
  if (!write_traj(traj_path, R.traj)) return 1;
  const int nf = n - 1;
  std::printf("{\"frames\": %d, \"ms_per_frame\": %.4f, \"frames_per_s\": %.2f, \"ms_track_call\": %.4f, \"ms_track_gpu\": %.4f, "
              "\"ms_frame_without_local_ba\": %.4f, \"local_bas\": %d, \"ms_per_local_ba\": %.4f, \"ms_per_key_frame_preintegration\": %.4f, \"ms_per_local_mapping_job\": %.4f, \"key_frames\": %zu, "
              "\"map_points\": %zu, \"widened\": %d, \"lba_lag\": %d, \"prefetch\": %d, \"ate_rmse_vs_truth_m\": %.6e, \"max_err_vs_truth_m\": %.6e, "
              "\"caller_ms_per_frame\": {\"map_write_back\": %.4f, \"of_which_waiting_for_local_mapping\": %.4f, \"before_call\": %.4f, \"after_call\": %.4f, \"key_frame_bookkeeping\": %.4f}, %s}\n",
              nf, rt.ms_total / nf, 1e3 * nf / rt.ms_total, R.ms_track / nf, R.ms_gpu / nf, R.ms_frames / nf, R.n_lba,
              R.n_lba ? R.ms_lba / R.n_lba : 0.0, R.n_lba ? R.ms_kf_preint / R.n_lba : 0.0, R.n_lba ? R.ms_lba_job / R.n_lba : 0.0, R.kfs.size(), R.mp_bad.size(), R.widened, lba_lag, prefetch, err.rmse, err.max,
              rt.ms_before / nf, R.ms_wait_lm / nf, R.ms_prep / nf, R.ms_post / nf, R.ms_finish / nf, R.run_shape_json().c_str());
  return 0;
}
