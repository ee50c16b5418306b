// ws_hold_check.cpp -- the call sequence of WsHold (csrc/internal.hpp), the only way to the context's shared workspace, on every kind
// of return path.  Host only: the hold's two HIP calls (ws_acquire / ws_release, mzk.hip in the library), cur(), set_error and
// hip_status are recording stubs here; needs the HIP headers, no HIP library and no device.
//   g++ -std=c++17 -pthread -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -I../mpc-jellyfish_amd/csrc -o ws_hold_check ws_hold_check.cpp && ./ws_hold_check
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "internal.hpp"

namespace mzk {
static std::vector<std::string> g_log;
static hipStream_t g_fail_on = nullptr;                     // the stream whose acquire fails (none: null is no stream of this program)
static Ctx g_ctx;
static std::string tag(const char* what, Workspace& ws, hipStream_t st) {
    return std::string(what) + (&ws == &g_ctx.ws ? ":" : ":FOREIGN-WORKSPACE:") + std::to_string((long)(intptr_t)st);
}
Ctx& cur() { return g_ctx; }
void set_error(const std::string&) {}
int32_t hip_status(hipError_t e, const char*) { return e == hipSuccess ? MZK_OK : MZK_ERR_HIP; }
int32_t ws_acquire(Workspace& ws, hipStream_t st) {
    if (st == g_fail_on) { g_log.push_back(tag("wait-failed", ws, st)); return MZK_ERR_HIP; }
    g_log.push_back(tag("wait", ws, st));
    return MZK_OK;
}
void ws_release(Workspace& ws, hipStream_t st) { g_log.push_back(tag("record", ws, st)); }
}  // namespace mzk

using namespace mzk;

// (f) one hold, one scope, one record: a copy or a move would record twice or on the wrong path
static_assert(!std::is_copy_constructible<WsHold>::value && !std::is_move_constructible<WsHold>::value, "WsHold must not be copy- or move-constructible");
static_assert(!std::is_copy_assignable<WsHold>::value && !std::is_move_assignable<WsHold>::value, "WsHold must not be assignable");

static const hipStream_t A = (hipStream_t)(intptr_t)1, B = (hipStream_t)(intptr_t)2;

static int32_t returns_normally(hipStream_t st) {
    WsHold ws; MZK_TRY(ws.acquire(st));
    if (&*ws != &g_ctx.ws || &ws->io != &g_ctx.ws.io) return -1000;       // the hold hands out the current context's workspace
    g_log.push_back("body");
    return MZK_OK;
}
static int32_t fails_midway(hipStream_t st) {
    WsHold ws; MZK_TRY(ws.acquire(st));
    g_log.push_back("body");
    MZK_TRY(MZK_ERR_OOM);                                                   // what a failing reserve() does at a call site
    g_log.push_back("NOT REACHED");
    return MZK_OK;
}
static int32_t nested(hipStream_t outer, hipStream_t inner) {
    WsHold ws; MZK_TRY(ws.acquire(outer));
    g_log.push_back("outer");
    MZK_TRY(returns_normally(inner));                                        // a dispatch inside a hold takes its own
    g_log.push_back("outer again");
    return MZK_OK;
}
static int32_t never_acquired(bool early) {
    WsHold ws;
    if (early) return MZK_ERR_INVALID_ARG;                                  // an argument check before the acquire
    return MZK_OK;
}

static int failures = 0;
static void expect(const char* name, int32_t rc, int32_t want_rc, const std::vector<std::string>& want) {
    const bool ok = rc == want_rc && g_log == want;
    std::printf("%-28s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) {
        failures++;
        std::printf("  rc %d (want %d); calls:", rc, want_rc);
        for (auto& s : g_log) std::printf(" [%s]", s.c_str());
        std::printf("\n");
    }
    g_log.clear();
}

int main() {
    expect("(a) normal return", returns_normally(A), MZK_OK, {"wait:1", "body", "record:1"});
    expect("(b) early return", fails_midway(A), MZK_ERR_OOM, {"wait:1", "body", "record:1"});
    g_fail_on = A;
    expect("(c) acquire fails", returns_normally(A), MZK_ERR_HIP, {"wait-failed:1"});
    g_fail_on = nullptr;
    expect("(d) nested, one stream", nested(A, A), MZK_OK, {"wait:1", "outer", "wait:1", "body", "record:1", "outer again", "record:1"});
    expect("(d') nested, two streams", nested(A, B), MZK_OK, {"wait:1", "outer", "wait:2", "body", "record:2", "outer again", "record:1"});
    g_fail_on = B;
    expect("(d'') inner acquire fails", nested(A, B), MZK_ERR_HIP, {"wait:1", "outer", "wait-failed:2", "record:1"});
    g_fail_on = nullptr;
    expect("(e) never acquired", never_acquired(false), MZK_OK, {});
    expect("(e') never acquired, early", never_acquired(true), MZK_ERR_INVALID_ARG, {});
    if (failures) std::printf("ws hold: %d case(s) FAILED\n", failures);
    else std::printf("ws hold: ok\n");
    return failures ? 1 : 0;
}
