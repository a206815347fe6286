// The one place where the library reads its environment.
#include "switches.h"
#include <stdlib.h>

namespace {
enum Kind { arm, value, live };
struct Row { const char* name; Kind kind; int def; };
// one row per LxoSwitch, in the enum's order
const Row kSwitches[SW_COUNT] = {
    {"LXO_ATT_ALT", arm, 1},
    {"LXO_ATT_EXP", arm, 1},
    {"LXO_BEAM_FAST", arm, 1},
    {"LXO_BEAM_INDIRECT", arm, 1},
    {"LXO_RSTEP_MT16", arm, 1},
    {"LXO_GEMM_NT_DMA", arm, 1},
    {"LXO_GEMM_TN_TR", arm, 1},
    {"LXO_WGRAD_HALO", arm, 1},
    {"LXO_POOL_FUSED", arm, 1},
    {"LXO_CONV1_MFMA", arm, 1},
    {"LXO_CONV_2WG", arm, 1},
    {"LXO_CONV_SMALL", value, 256},
    {"LXO_XDEC", arm, 1},
    {"LXO_XDEC_DEC", arm, 1},
    {"LXO_XDEC_BWD", arm, 1},
    {"LXO_XDEC_DEC_CHUNK", live, 0},
};
int read(const Row& r) {
    const char* e = getenv(r.name);
    if (!e) return r.def;
    return r.kind == arm ? e[0] != '0' : atoi(e);
}
struct Cache {
    int v[SW_COUNT];
    Cache() { for (int i = 0; i < SW_COUNT; ++i) v[i] = read(kSwitches[i]); }
};
}  // namespace

int lxo_switch(LxoSwitch s) {
    static const Cache cache;      // filled once, under the lock of a function-local static: no thread sees a half-read table
    return kSwitches[s].kind == live ? read(kSwitches[s]) : cache.v[s];
}
#ifdef LXO_DIAG
int lxo_conv_diag() {
    static const int diag = [] { const char* e = getenv("LXO_CONV_DIAG"); return e ? atoi(e) : 0; }();
    return diag;
}
#endif
