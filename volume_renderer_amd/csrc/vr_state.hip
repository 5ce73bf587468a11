// vr_state.hip -- the one definition of everything the host files share (vr_host.h): the module-global
// texture unit and its lock, the handle set, the switches, the last error and launch flags, the pool of
// group streams; and what the kernel files' launchers call back for.
#include "vr_host.h"

namespace vr_host {
std::atomic<int> g_test_switches{0};
}
namespace vr {
bool test_switches_on() { return vr_host::g_test_switches.load() != 0; }
std::string &last_march_kernel() {
  static std::string name;
  return name;
}

void note_march_kernel(bool fast, int K, int mode, bool ab, bool count, bool share, bool big, int cap, int sched,
                       int nl) {
  char b[160];
  auto tf = [](bool v) { return v ? "true" : "false"; };
  std::snprintf(b, sizeof b, "vr::%s::march_kernel<%d, %d, %s, %s, %s, %s, %d, %d, %d>", fast ? "fast" : "exact", K,
                mode, tf(ab), tf(count), tf(share), tf(big), cap, sched, nl);
  last_march_kernel() = b;
}
}  // namespace vr

namespace vr_host {

uint32_t g_last_launch_flags = 0;

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

std::mutex g_mu;
// The module state and the resource lists of vr_resources.h are never destroyed: at process exit
// their destructors would run in an order unrelated to their use (a binding's buffer returning its
// memory to an already destroyed pool, events destroyed after the runtime's own teardown) -- the
// process exit releases the device memory anyway.
TexUnit &g_tex = *new TexUnit();
static uint64_t g_version = 0;
uint64_t next_version() { return ++g_version; }
std::set<vr_context *> g_contexts;

bool valid(vr_context *h) { return h && g_contexts.count(h) && h->signature == 0xFF00F0A5u; }

bool env_flag(const char *name) {
  const char *ev = std::getenv(name);
  return ev && ev[0] == '1';
}
bool env_flag_off(const char *name) {
  const char *ev = std::getenv(name);
  return ev && ev[0] == '0';
}
// A/B and diagnostic switches (INTEGRATION.md "Runtime switches"): read by a DIAG=1 build only
// (Makefile; -DVR_DIAG=1), ignored by the default library
#ifndef VR_DIAG
#define VR_DIAG 0
#endif
const char *diag_env(const char *name) { return VR_DIAG ? std::getenv(name) : nullptr; }
bool diag_flag(const char *name) {
  const char *ev = diag_env(name);
  return ev && ev[0] == '1';
}
// Test switches (round 6, INTEGRATION.md "Runtime switches"): the kernel-variant and schedule
// switches the GPU tests and the measurement tools set through the environment are read only after
// vr_set_option("test_switches", 1) (tests/conftest.py, bench.py diagnostics, tools/) or in a DIAG=1
// build, so that a MATLAB session's environment never selects them.  The production switches
// (VR_EXACT_SHADE, VR_ALWAYS_REUPLOAD, VR_GROUP_PEER, the upload ring's) are read always.
const char *test_env(const char *name) { return (VR_DIAG || g_test_switches.load()) ? std::getenv(name) : nullptr; }
bool test_flag(const char *name) {
  const char *ev = test_env(name);
  return ev && ev[0] == '1';
}
bool test_flag_off(const char *name) {
  const char *ev = test_env(name);
  return ev && ev[0] == '0';
}

// Group streams are never destroyed.  Events recorded on them (replica copies, group renders) live on
// after the group is deleted -- in the reader lists of buffers that stay bound, pooled or retired --
// and a later query of such an event reads the runtime's stream object: destroyed, that read gave
// spurious stream-capture errors (hipErrorCapturedEvent / hipErrorStreamCaptureUnsupported from
// unrelated calls, intermittently).  A deleted group's streams wait here for the next group.
static std::map<int, std::vector<hipStream_t>> &idle_streams() {
  static std::map<int, std::vector<hipStream_t>> &m = *new std::map<int, std::vector<hipStream_t>>();
  return m;
}
hipError_t take_stream(int dev, hipStream_t *s) {  // dev is current
  std::vector<hipStream_t> &v = idle_streams()[dev];
  if (!v.empty()) {
    *s = v.back();
    v.pop_back();
    return hipSuccess;
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
void give_stream(int dev, hipStream_t s) {  // s is idle
  if (s) idle_streams()[dev].push_back(s);
}

}  // namespace vr_host
