// host_paths_check.cpp — the host side of the C ABI (smplsim_amd/csrc/ss_api.h) on a backend without a device, for a
// run under AddressSanitizer / UBSan (tests/test_host_paths_sanitized.py builds and runs it): model and batch creation, every
// setter, a refused and an accepted ss_imitation_bind, a model of three body shapes, teardown — once with every allocation and upload
// succeeding, then again with the n-th one failing, for every n until a run makes no failing call; before that, every description that
// model creation refuses.  Any leak, double free or undefined behaviour on one
// of these paths ends the program with the sanitizer's report.  usage: host_paths_check MJCF_FILE
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../smplsim_amd/csrc/ss_api.h"

namespace {

struct FakeBackend {                                         // alloc = malloc, launches do nothing
  static inline long calls = 0, fail_at = -1;                // the fail_at-th alloc / upload of a run fails (-1: none)
  static inline bool failed = false;
  static bool trip() { const bool f = calls++ == fail_at; failed |= f; return f; }
  static void *alloc(size_t n) { return trip() ? nullptr : malloc(n); }
  static void free_(void *p) { free(p); }
  static bool upload(void *dst, const void *src, size_t n) { if (trip()) return false; memcpy(dst, src, n); return true; }
  static bool download(void *dst, const void *src, size_t n) { memcpy(dst, src, n); return true; }
  static bool copy_d2d(void *, const void *, size_t, void *) { return true; }
  static bool set_device(int) { return true; }
  static int lds_capacity() { return 160 * 1024; }
  static int max_waves(int, int) { return 16; }
  static int kernel_regs() { return 0; }
  static const char *order_by_key(const ss_state &, int, int32_t *, int32_t *, void *) { return nullptr; }
  static const char *gae(const float *, const float *, const float *, const float *, const float *, int, int, float, float, float *, float *, void *) { return nullptr; }
  static const char *launch(const ss::KArgs &, int, int, size_t, void *, int, int) { return nullptr; }
};

}  // namespace

SS_DEFINE_C_API(FakeBackend)

namespace {

[[noreturn]] void die(const char *what) { fprintf(stderr, "host_paths_check: %s (ss_last_error: %s)\n", what, ss_last_error()); exit(1); }

// a call that may only fail because this run's allocation / upload failure was injected, and then with a message
bool went(int rc, const char *what) {
  if (rc == SS_OK) return true;
  if (!FakeBackend::failed || !*ss_last_error()) die(what);
  return false;
}

alignas(16) float nowhere[16];                               // stands for every caller-owned device buffer: nothing here follows one
template <class T> T *buf() { return reinterpret_cast<T *>(nowhere); }

ss_state state_of(int n, bool shaped) {
  ss_state st{};
  st.num_envs = n;
  st.qpos = st.qvel = st.qpos_prev = st.qvel_prev = st.qacc_warm = st.body_vel = st.task = buf<float>();
  st.touch = st.cur_t = st.nwarn = st.solver_iters = buf<int32_t>();
  st.shape_id = shaped ? buf<int32_t>() : nullptr;
  return st;
}

void every_setter(ss_batch *b) {
  if (ss_set_order(b, buf<int32_t>()) || ss_set_launch_geometry(b, 1, 2) || ss_set_body_outputs(b, buf<float>(), buf<float>()) ||
      ss_set_power_output(b, buf<float>()) || ss_debug_self_truncation(b, buf<int32_t>()) || ss_debug_self_contacts(b, buf<float>()) ||
      ss_set_fall_actions(b, buf<float>()))
    die("a setter failed");
  if (ss_set_body_outputs(b, buf<float>(), nullptr) != SS_ERR_INVALID || strcmp(ss_batch_last_error(b), "pass both buffers or neither")) die("ss_set_body_outputs took one buffer");
}

void run(const std::string &xml, const ss_model_desc *descs) {
  // one shape, StateInit External: everything an imitation batch allocates
  ss_model *m = nullptr;
  if (went(ss_model_create_from_mjcf(xml.data(), xml.size(), nullptr, 0, &m), "ss_model_create_from_mjcf")) {
    int32_t nb = 0;
    if (ss_model_dims(m, nullptr, nullptr, nullptr, &nb) || nb < 1) die("ss_model_dims");
    ss_env_cfg cfg{};
    cfg.task = SS_TASK_BASE; cfg.state_init = SS_INIT_EXTERNAL; cfg.self_obs_v = 1; cfg.control_mode = SS_CTRL_UHC_PD; cfg.control_freq_inv = 15;
    const ss_state st = state_of(4, false);
    ss_batch *b = nullptr;
    if (went(ss_batch_create(m, &cfg, &st, &b), "ss_batch_create")) {
      every_setter(b);
      ss_motion_data d{};
      d.num_motions = d.num_frames = 1; d.nbody = nb;
      d.length_starts = d.motion_num_frames = buf<int32_t>(); d.motion_dt = d.motion_lengths = buf<float>();
      d.gts = d.grs = d.gvs = d.gavs = d.dof_pos = d.dvs = d.qpos = d.qvel = buf<float>();
      ss_imitation_io io{};
      io.data = &d; io.motion_ids = buf<int32_t>(); io.start_times = io.obs_final = io.obs_next = io.reward = buf<float>();
      io.terminated = io.truncated = buf<uint8_t>(); io.obs_stride = ss_obs_size(m, &cfg) + 24 * nb;
      if (went(ss_imitation_bind(b, &io), "ss_imitation_bind") && ss_imitation_step_fused(b, buf<float>(), nullptr, nullptr)) die("ss_imitation_step_fused");
      went(ss_schedule_longest_first(b, nullptr), "ss_schedule_longest_first");
      if (ss_step(b, buf<float>(), nullptr, buf<float>(), buf<float>(), buf<uint8_t>(), buf<uint8_t>(), nullptr)) die("ss_step");
      ss_batch_destroy(b);
    } else if (b) die("ss_batch_create failed and handed a batch out");
    ss_model_destroy(m);
  } else if (m) die("ss_model_create_from_mjcf failed and handed a model out");

  // two body shapes, StateInit Default: ss_imitation_bind refuses the batch
  ss_model *m2 = nullptr;
  if (went(ss_model_create_shapes(descs, 2, 0, &m2), "ss_model_create_shapes")) {
    ss_env_cfg cfg{};
    cfg.task = SS_TASK_BASE; cfg.state_init = SS_INIT_DEFAULT; cfg.self_obs_v = 1; cfg.control_mode = SS_CTRL_UHC_PD; cfg.control_freq_inv = 15;
    const ss_state st = state_of(4, true);
    ss_batch *b = nullptr;
    if (went(ss_batch_create(m2, &cfg, &st, &b), "ss_batch_create (shapes)")) {
      every_setter(b);
      ss_motion_data d{};
      d.num_motions = d.num_frames = 1; d.nbody = descs[0].nbody;
      d.length_starts = d.motion_num_frames = buf<int32_t>(); d.motion_dt = d.motion_lengths = buf<float>();
      d.gts = d.grs = d.gvs = d.gavs = d.dof_pos = d.dvs = d.qpos = d.qvel = buf<float>();
      ss_imitation_io io{};
      io.data = &d;
      if (ss_imitation_bind(b, &io) != SS_ERR_INVALID || strcmp(ss_batch_last_error(b), "the fused imitation step needs a batch with task base and StateInit External"))
        die("ss_imitation_bind took a batch that is not StateInit External");
      ss_batch_destroy(b);
    } else if (b) die("ss_batch_create failed and handed a batch out");
    ss_model_destroy(m2);
  } else if (m2) die("ss_model_create_shapes failed and handed a model out");

  // three body shapes: per-shape tables concatenated, six tables uploaded
  ss_model *m3 = nullptr;
  if (went(ss_model_create_shapes(descs, 3, 0, &m3), "ss_model_create_shapes (3 shapes)")) ss_model_destroy(m3);
  else if (m3) die("ss_model_create_shapes failed and handed a model out");
}

// every description that model creation refuses: one change to a good description at a time, the code and the message, nothing handed out
void refusals(ss::mjcf::Compiled *c, ss_model_desc *d) {      // d[i]: a copy of c[i].desc, its arrays are c[i]'s
  auto refused = [&](int num_shapes, const char *msg) {
    ss_model *m = nullptr;
    const int rc = num_shapes == 1 ? ss_model_create(d, 0, &m) : ss_model_create_shapes(d, num_shapes, 0, &m);
    if (rc != SS_ERR_INVALID || m || strcmp(ss_last_error(), msg)) { fprintf(stderr, "expected the refusal \"%s\"\n", msg); die("a refusal went wrong"); }
  };
  auto with = [&](auto &slot, auto value, int num_shapes, const char *msg) { const auto old = slot; slot = value; refused(num_shapes, msg); slot = old; };
  with(d->nbody, 0, 1, "nbody must be in [1,63]");
  with(c[0].parent[0], 0, 1, "body 0 must be the root");
  with(c[0].parent[1], 1, 1, "parents must precede children");
  with(c[0].parent[9], 1, 1, "bodies must be in depth-first order");          // body 8 is the end of the right leg: 1 is none of its ancestors
  with(c[0].arm[2], 0.01, 1, "armature on the free joint is not supported");
  with(c[0].adof[0], 5, 1, "bad actuator_dof");
  with(c[0].gtype[3], 5, 1, "unknown geom type");
  with(d->impratio, 2.0, 1, "impratio != 1 is not supported");
  with(c[1].kp[3], 2 * c[1].kp[3], 2, "shape 1 differs from shape 0 in more than its geometry");
  with(d[2].impratio, 2.0, 3, "shape 2: impratio != 1 is not supported");
  const std::vector<int32_t> parents = c[0].parent;         // a star: every rooting has a level of more than 16 bodies
  std::fill(c[0].parent.begin() + 1, c[0].parent.end(), 0);
  refused(1, "more than 16 nodes in one tree level");
  std::copy(parents.begin(), parents.end(), c[0].parent.begin());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s MJCF_FILE\n", argv[0]); return 2; }
  std::stringstream text;
  text << std::ifstream(argv[1]).rdbuf();
  const std::string xml = text.str();
  if (xml.empty()) { fprintf(stderr, "host_paths_check: cannot read %s\n", argv[1]); return 2; }
  ss::mjcf::Compiled c[3]; std::string e;                    // the body shapes of ss_model_create_shapes: geom sizes and body offsets scaled
  for (auto &ci : c) if (!ss::mjcf::compile(xml.data(), xml.size(), nullptr, ci, e)) die(e.c_str());
  for (double &x : c[1].gsize) x *= 0.9;
  for (double &x : c[1].pos) x *= 0.9;
  for (double &x : c[2].gsize) x *= 1.1;
  for (double &x : c[2].pos) x *= 1.1;
  ss_model_desc descs[3] = {c[0].desc, c[1].desc, c[2].desc};
  refusals(c, descs);
  FakeBackend::calls = 0;
  run(xml, descs);                                           // nothing fails
  if (FakeBackend::failed) die("a failure without one injected");
  const long total = FakeBackend::calls;
  long n = 0;
  for (;; n++) {                                             // the n-th alloc / upload fails
    FakeBackend::calls = 0; FakeBackend::fail_at = n; FakeBackend::failed = false;
    run(xml, descs);
    if (!FakeBackend::failed) break;
  }
  printf("host_paths_check: %ld allocations and uploads in the full run, %ld failing runs\n", total, n);
  return n == total ? 0 : 1;
}
