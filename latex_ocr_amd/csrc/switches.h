// The library's environment switches: ONE table (switches.hip), one accessor.  No other translation unit reads the environment.
// DESIGN.md ("Environment switches") lists what each switch's other arm is and which test holds it.
#pragma once

enum LxoSwitch {
    SW_ATT_ALT, SW_ATT_EXP, SW_BEAM_FAST, SW_BEAM_INDIRECT, SW_RSTEP_MT16, SW_GEMM_NT_DMA, SW_GEMM_TN_TR, SW_WGRAD_HALO,
    SW_POOL_FUSED, SW_CONV1_MFMA, SW_CONV_2WG, SW_CONV_SMALL, SW_XDEC, SW_XDEC_DEC, SW_XDEC_BWD, SW_XDEC_DEC_CHUNK,
    SW_COUNT
};
// arm: 1, or 0 when the variable is set and begins with '0'.  value: atoi of the variable, or the default.  Both are read once per
// process; a live switch is read again on every call.
int lxo_switch(LxoSwitch s);
#ifdef LXO_DIAG
int lxo_conv_diag();
#endif
