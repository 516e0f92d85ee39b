// Stand-alone host check of the activity gate's entry points (csrc/frame_activity.hip): every refusal the header lists must
// come back as FR_E_INVALID with a message, and N == 0 as FR_OK, before anything is launched - so the program needs no GPU and
// never makes a call that would reach a launch.  Meant to be built with the host sanitizers, from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       facerecognition_infrenceengine_amd/csrc/frame_activity.hip tools/activity_refusals_main.cpp -o activity_refusals
//   ./activity_refusals
//
// It brings its own fr_set_error (csrc/abi.cpp has the library's), so nothing else of the library is linked.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include "../include/frhip.h"

static char g_err[512] = "";

void fr_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

int failures = 0;
uint8_t bytes[64];
int32_t words[16];

struct Args {
    const uint8_t* frames = bytes;
    const fr_frame_ref* refs = reinterpret_cast<const fr_frame_ref*>(bytes);
    int N = 1, H = 32, W = 48;
    const int32_t* slot = words;
    int S = 4;
    uint8_t* grid = bytes;
    int32_t *geom = words, *idle = words;
    int C = 6;
    uint8_t* cur = bytes;
    int32_t *changed = words, *active = words;
    int thr = 4, min_cells = 2, max_idle = 0;
};

int uniform(const Args& a) {
    return fr_frame_activity_u8(a.frames, a.N, a.H, a.W, a.slot, a.S, a.grid, a.geom, a.idle, a.C, a.cur, a.changed, a.active, a.thr,
                                a.min_cells, a.max_idle, nullptr);
}

int table(const Args& a) {
    return fr_frame_activity_refs_u8(a.refs, a.N, a.slot, a.S, a.grid, a.geom, a.idle, a.C, a.cur, a.changed, a.active, a.thr,
                                     a.min_cells, a.max_idle, nullptr);
}

void expect(const char* what, int rc, int want) {
    const bool ok = rc == want && (want == FR_OK || g_err[0] != 0);
    std::printf("%-58s rc %2d  %s%s\n", what, rc, ok ? "ok" : "WRONG", want == FR_OK ? "" : (std::string(" | ") + g_err).c_str());
    if (!ok) ++failures;
    g_err[0] = 0;
}

template <class F>
void both(const char* what, F&& change, bool uniform_only = false) {
    Args a;
    change(a);
    char name[96];
    std::snprintf(name, sizeof(name), "uniform: %s", what);
    expect(name, uniform(a), FR_E_INVALID);
    if (uniform_only) return;
    std::snprintf(name, sizeof(name), "table:   %s", what);
    expect(name, table(a), FR_E_INVALID);
}

}  // namespace

int main() {
    both("N = -1", [](Args& a) { a.N = -1; });
    both("N = 65536", [](Args& a) { a.N = 65536; });
    both("S = 0", [](Args& a) { a.S = 0; });
    both("C = -1", [](Args& a) { a.C = -1; });
    both("thr = -1", [](Args& a) { a.thr = -1; });
    both("thr = 256", [](Args& a) { a.thr = 256; });
    both("min_cells = 0", [](Args& a) { a.min_cells = 0; });
    both("max_idle = -1", [](Args& a) { a.max_idle = -1; });
    both("H = 0", [](Args& a) { a.H = 0; }, true);
    both("W = -3", [](Args& a) { a.W = -3; }, true);
    both("H * W * 3 = 2^31 + 1", [](Args& a) { a.H = 1; a.W = 715827883; }, true);
    both("32768 x 32768", [](Args& a) { a.H = a.W = 32768; }, true);
    both("frames null", [](Args& a) { a.frames = nullptr; a.refs = nullptr; });
    both("slot null", [](Args& a) { a.slot = nullptr; });
    both("grid null", [](Args& a) { a.grid = nullptr; });
    both("geom null", [](Args& a) { a.geom = nullptr; });
    both("idle null", [](Args& a) { a.idle = nullptr; });
    both("cur null", [](Args& a) { a.cur = nullptr; });
    both("changed null", [](Args& a) { a.changed = nullptr; });
    both("active null", [](Args& a) { a.active = nullptr; });
    Args none;
    none.N = 0;
    none.frames = nullptr; none.refs = nullptr; none.slot = nullptr; none.grid = nullptr; none.geom = nullptr; none.idle = nullptr;
    none.cur = nullptr; none.changed = nullptr; none.active = nullptr;
    expect("uniform: N = 0, every pointer null", uniform(none), FR_OK);
    expect("table:   N = 0, every pointer null", table(none), FR_OK);
    none.thr = 255; none.min_cells = 2147483647; none.max_idle = 2147483647;
    expect("uniform: N = 0, the edges of the ranges", uniform(none), FR_OK);
    expect("table:   N = 0, the edges of the ranges", table(none), FR_OK);
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
