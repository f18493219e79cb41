// abi.cpp — version / error plumbing of the C ABI (include/mumpy_hip.h and every mumpy_hip_ext*.h: each header's version function).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "common.h"
#include "../../include/mumpy_hip_ext.h"
#include "../../include/mumpy_hip_ext2.h"
#include "../../include/mumpy_hip_ext3.h"
#include "../../include/mumpy_hip_ext4.h"
#include "../../include/mumpy_hip_ext5.h"
#include "../../include/mumpy_hip_ext6.h"
#include "../../include/mumpy_hip_ext7.h"
#include "../../include/mumpy_hip_ext8.h"
#include "../../include/mumpy_hip_ext9.h"
#include "../../include/mumpy_hip_ext10.h"
#include "../../include/mumpy_perturb.h"
#include "../../include/mumpy_photometric.h"
#include "../../include/mumpy_geometric.h"
#include "../../include/mumpy_postprocess.h"

namespace mumpy {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
thread_local Route g_route;
static thread_local char g_route_text[160] = "";
static const char* format_route() {
    static const char* const addr[] = {"dense", "rows", "kseg", "conv"};
    static const char* const ln[] = {"none", "producer", "consumer"};
    static const char* const red[] = {"none", "one", "two-in-one", "taps"};
    const Route& r = g_route;
    char* t = g_route_text;
    const size_t n = sizeof(g_route_text);
    switch (r.family) {
    case Route::TILED: snprintf(t, n, "tiled tile=%d ks=%d np=%d addr=%s", r.tile, r.ks, r.np, addr[r.addr & 3]); break;
    case Route::TILED16: snprintf(t, n, "tiled16 tile=%d ks=%d np=%d addr=%s", r.tile, r.ks, r.np, addr[r.addr & 3]); break;
    case Route::WS:
        snprintf(t, n, "ws sched=%s P=%d ln=%s addr=%s", r.split ? "split" : "whole", r.passes, ln[r.ln < 3 ? r.ln : 0], addr[r.addr & 3]);
        break;
    case Route::WS64: snprintf(t, n, "ws64 P=%d addr=dense", r.passes); break;
    case Route::WS16: snprintf(t, n, "ws16 P=%d addr=dense", r.passes); break;
    case Route::XGEMM: {
        char dx[24] = "-", dw[24] = "-";
        if (r.prod[0].wt) snprintf(dx, sizeof(dx), "%dx%d", r.prod[0].wt, r.prod[0].ks);
        if (r.prod[1].wt) snprintf(dw, sizeof(dw), "%dx%d", r.prod[1].wt, r.prod[1].ks);
        snprintf(t, n, "xgemm np=%d addr=%s dx=%s dw=%s reduce=%s", r.np, addr[r.addr & 3], dx, dw, red[r.reduce & 3]);
        break;
    }
    default: snprintf(t, n, "none");
    }
    // the dual-output forward (z beside a = gelu(z)) / the backward whose dX carries gelu'(z): a marker behind the sibling's text
    if (r.dual && r.family != Route::NONE) {
        const size_t len = strlen(t);
        snprintf(t + len, n - len, r.family == Route::XGEMM ? " gate=gelu" : " dual=z");
    }
    return t;
}
#ifdef MUMPY_TUNING
#include <stdlib.h>
int tune_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
const char* tune_str(const char* name) { return getenv(name); }
#endif
}  // namespace mumpy

// 1 when this library was built with the tuning hooks (reads MUMPY_* environment variables), 0 for the shipped build
extern "C" int mumpy_tuning_build(void) {
#ifdef MUMPY_TUNING
    return 1;
#else
    return 0;
#endif
}

extern "C" int mumpy_abi_version(void) { return MUMPY_ABI_VERSION; }
extern "C" int mumpy_ext_version(void) { return MUMPY_EXT_VERSION; }
extern "C" int mumpy_ext2_version(void) { return MUMPY_EXT2_VERSION; }
extern "C" int mumpy_ext3_version(void) { return MUMPY_EXT3_VERSION; }
extern "C" int mumpy_ext4_version(void) { return MUMPY_EXT4_VERSION; }
extern "C" int mumpy_ext5_version(void) { return MUMPY_EXT5_VERSION; }
extern "C" int mumpy_ext6_version(void) { return MUMPY_EXT6_VERSION; }
extern "C" int mumpy_ext7_version(void) { return MUMPY_EXT7_VERSION; }
extern "C" int mumpy_ext8_version(void) { return MUMPY_EXT8_VERSION; }
extern "C" int mumpy_ext9_version(void) { return MUMPY_EXT9_VERSION; }
extern "C" int mumpy_ext10_version(void) { return MUMPY_EXT10_VERSION; }
extern "C" int mumpy_perturb_version(void) { return MUMPY_PERTURB_VERSION; }
extern "C" int mumpy_photometric_version(void) { return MUMPY_PHOTOMETRIC_VERSION; }
extern "C" int mumpy_geometric_version(void) { return MUMPY_GEOMETRIC_VERSION; }
extern "C" int mumpy_postprocess_version(void) { return MUMPY_POSTPROCESS_VERSION; }
extern "C" const char* mumpy_last_error(void) { return mumpy::g_err; }
extern "C" const char* mumpy_last_route(void) { return mumpy::format_route(); }
