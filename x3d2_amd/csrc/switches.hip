// The library's environment switches: the one table of their names and the one place that reads the environment.
// x3d_backend_create resolves them into b->sw (common.h), x3d_backend_create_like copies them; nothing that runs per call
// looks at the environment.  (X3D_ROCTX alone is read in prof.hip: it belongs to the process, not to a backend.)
// Host code only.
#include <cstdlib>

#include "common.h"

enum SwKind {
    SW_FLAG,  // 1 when the value's first character is '1'
    SW_INT,   // atoi of the value; `unset` when the variable is not there
    SW_MASK,  // strtoul of the value, base 0; `unset` when the variable is not there
    SW_FORM,  // X3D_Y010_FORM: unset or empty = `unset`, a value that begins "st" = 1 (staged), anything else = 0 (split)
};
struct SwEntry {
    const char *name;
    SwKind kind;
    long unset;
    long x3d_switches::*field;
};
#define F(name, field) {name, SW_FLAG, 0, &x3d_switches::field}
static const SwEntry g_table[] = {
    F("X3D_NO_XSCAN", no_xscan),                  // x: the generic (lane-per-pencil) kernels instead of the wave-per-pencil ones
    F("X3D_XDIR_GENERIC", xdir_generic),          // x: the direction-generic two-sweep kernels
    F("X3D_XSCAN_P1", xscan_p1),                  // x transeq: one pencil per wave
    F("X3D_NO_TILE3", no_tile3),                  // transeq: one launch per component
    F("X3D_NO_XCIRC", no_xcirc),                  // x kernels: lane tables instead of the circulant solve
    F("X3D_NO_CIRC", no_circ),                    // every kernel: lane tables instead of the circulant solve
    F("X3D_NO_HALO_CIRC", no_halo_circ),          // HALO forms: the table form
    F("X3D_NO_UNIFORM", no_uniform),              // the general tables on uniform grids too
    F("X3D_NO_TDS_LINCOMB", no_tds_lincomb),      // x: tds_solve and the linear combination as two launches
    F("X3D_NO_XWIDE", no_xwide),                  // 1024-row x pencils through the generic kernels
    F("X3D_NO_XWIDE_UPD", no_xwide_upd),          // 1024-row x transeq without the velocity correction folded in
    F("X3D_NO_VIA_X", no_via_x),                  // y / z: two-sweep kernels
    F("X3D_NO_YTILE", no_ytile),                  // y / z: through transposed copies instead of the tile kernels
    F("X3D_NO_ZTILE", no_ztile),                  // z only: through transposed copies instead of the tile kernels
    F("X3D_NO_YGEN", no_ygen),                    // y / z pencils of general length: not through the tile kernels
    F("X3D_NO_Q5", no_q5),                        // 257..320-row pencils: the operators' own rows per lane, never 5
    F("X3D_NO_DIRECT", no_direct),                // non-periodic one-rank operators: never the plain Thomas factors
    F("X3D_NO_TDS_PAIR", no_tds_pair),            // y / z: one operator per launch
    F("X3D_NO_NPW2", no_npw2),                    // FP32 tile kernels: one pencil per wave
    F("X3D_NO_ONCHIP2", no_onchip2),              // periodic 512-row y / z pencils: the two-sweep pair
    F("X3D_NO_SPECTRAL_PAD", no_spectral_pad),    // Poisson: dense spectral rows
    F("X3D_NO_FFT512", no_fft512),                // Poisson 512^3: rocFFT's 3-D plans
    F("X3D_NO_RWT", no_rwt),                      // Poisson 512^3: spectral division through the LDS tile, no z-fastest reciprocal wave numbers
    F("X3D_NO_R2C512", no_r2c512),                // Poisson with 512-point x rows: rocFFT's real-to-complex x pass
    F("X3D_NO_ZFIRST", no_zfirst),                // Poisson: no z-first solve on offer
    F("X3D_NO_XFFT_DIV", no_xfft_div),            // z-first 000 solve: its forward x transform as a pass of its own, not in the divergence's x operators
    F("X3D_NO_XFFT_GRAD", no_xfft_grad),          // z-first 000 solve: its inverse x transform as a pass of its own, not in the gradient's x operators
    F("X3D_NO_ZFIRST010", no_zfirst010),          // the channel's 010 solve: its x-first form
    F("X3D_NO_Y010", no_y010),                    // Poisson 010: the 3-D transforms with post-processing kernels between them
    F("X3D_Y010_NO_DB", y010_no_db),              // Poisson 010: the y pass without double buffering
    F("X3D_SFFT010_SPLIT_XY", sfft010_split_xy),  // slab 010 solver: x and y transforms as two plans
    F("X3D_NO_SLAB_FUSED_Z", no_slab_fused_z),    // slab solver: rocFFT along z
    F("X3D_LAZY_DUMP", lazy_dump),                // deferred execution: print each queue as recorded and as rewritten
    F("X3D_LAZY_REPORT", lazy_report),            // deferred execution: every counter on stderr when the process ends
    F("X3D_LAZY_KEEP_ZERO_TERMS", lazy_keep_zero_terms),  // deferred execution: keep the terms whose coefficient is zero
    {"X3D_LAZY_RULES", SW_MASK, 0xffffffffL, &x3d_switches::lazy_rules},  // deferred execution: mask of the rewrite rules that are on
    {"X3D_PAD_X", SW_INT, X3D_SW_UNSET, &x3d_switches::pad_x},            // doubles of row padding (backend.hip has the rule)
    {"X3D_SLAB_Z_SPLIT", SW_INT, -1, &x3d_switches::slab_z_split},       // > 0: the DFTs across z chunks as streaming passes
    {"X3D_Y010_FORM", SW_FORM, 1, &x3d_switches::y010_form},              // Poisson 010 y pass: "split" or "staged"; default staged (y010.hip has the measurements)
};
#undef F

static long resolve(const SwEntry &s)
{
    const char *e = getenv(s.name);
    switch (s.kind) {
    case SW_FLAG: return e && e[0] == '1';
    case SW_INT: return e ? atoi(e) : s.unset;
    case SW_MASK: return e ? (long)(unsigned)strtoul(e, nullptr, 0) : s.unset;
    default: return !e || !e[0] ? s.unset : (e[0] == 's' && e[1] == 't' ? 1 : 0);
    }
}

void x3d_switches_from_env(x3d_switches *sw)
{
    for (const SwEntry &s : g_table) sw->*s.field = resolve(s);
    sw->via_x = !(sw->no_via_x || sw->no_xscan);
    sw->ytile = sw->via_x && !sw->no_ytile;
    sw->ygen = sw->ytile && !sw->no_ygen;
    sw->x_fast = !(sw->no_xscan || sw->xdir_generic);
    sw->x_tq3 = sw->x_fast && !(sw->no_tile3 || sw->xscan_p1);
    sw->x_circ = !(sw->no_circ || sw->no_xcirc);
}

// the resolved value of a declared switch: b's, or with b == NULL what x3d_backend_create would store now (no GPU needed)
extern "C" int x3d_backend_switch(const x3d_backend *b, const char *name, long *value)
{
    X3D_REQUIRE(name && value, "x3d_backend_switch: null argument");
    for (const SwEntry &s : g_table)
        if (!strcmp(s.name, name)) {
            *value = b ? b->sw.*s.field : resolve(s);
            return 0;
        }
    x3d_set_error("x3d_backend_switch: %s is not a switch of the library", name);
    return 2;
}
