// The one order in which the kernel-level entries of the GEMM family (ams_k_pointwise*, ams_k_pack_h2i), the depthwise and stem family
// (ams_k_depthwise3x3*, ams_k_stem_conv) and the recompute family (ams_k_xdw_*, ams_k_xx_gram, ams_k_expand_stats) refuse a call, in front of
// their first launch (the weight splits are launches).  What block_call_check is to the frozen-block entries.  Host code only.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "kernels.hpp"

namespace ams {

// An entry fills this in from its arguments alone (comparisons and pure host functions: nothing is read through a pointer) and hands it to
// entry_check.  `need` is evaluated by the caller only once sizes and shape hold: the *_scratch() formulas divide by what the shape rule bounds.
struct EntryCall {
    const char* who = "";
    char dims[200] = "";                        // the arguments in words, for the messages
    bool sizes = true;                          // 1. every extent (B, H, W, M, K, N, C ...) > 0
    bool shape = true;                          // 2. the entry's shape rule
    const char* scratch_what = nullptr;         // 3. "scratch" | "panel scratch"; nullptr: the entry has none
    const void* scratch = nullptr; size_t have = 0, need = 0;
    bool scale_without_shift = false;           // 4.
    bool ptrs = true;                           // 5. every pointer the entry reads or writes
    void describe(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(dims, sizeof(dims), fmt, ap);
        va_end(ap);
    }
    bool shaped() const { return sizes && shape; }        // the scratch formula may be evaluated
};

// Refused in this order: no pixels or rows; the shape rule; scratch or panels NULL or too small; scale without shift; a null pointer.
static inline int entry_check(const EntryCall& c) {
    AMS_REQUIRE(c.sizes, "%s: empty problem (no pixels or rows): %s", c.who, c.dims);
    AMS_REQUIRE(c.shape, "%s: unsupported shape: %s", c.who, c.dims);
    AMS_REQUIRE(!c.scratch_what || (c.need != (size_t)-1 && c.scratch && c.have >= c.need), "%s: %s too small (need %zu): %s", c.who, c.scratch_what,
                c.need, c.dims);
    AMS_REQUIRE(!c.scale_without_shift, "%s: scale without shift", c.who);
    AMS_REQUIRE(c.ptrs, "%s: null pointer", c.who);
    return AMS_OK;
}

// ---- the shape rules, one per family (include/ams_hip.h states them next to the prototypes)
static inline bool dw_entry_shape(int C, int stride, int rate) {
    return C % 4 == 0 && C >= 4 && C <= 1024 && (stride == 1 || stride == 2) && (rate == 1 || rate == 2) && !(stride == 2 && rate == 2);
}
static inline bool frame_dtype_ok(int dtype) { return dtype == AMS_DT_U8 || dtype == AMS_DT_F32; }
// an image whose elements the recompute kernels address with 32-bit offsets
static inline bool xdw_image_ok(int H, int W, int Cin, int Cexp) { return (int64_t)H * W * (Cexp > Cin ? Cexp : Cin) < 0x7fffffffLL; }
static inline bool xdw_dwe_shape(int Cin, int Cexp) { return Cin >= 1 && Cin <= 32 && Cexp % 16 == 0 && Cexp >= 32 && Cexp <= 192; }
static inline bool xx_gram_shape(int Cin) { return Cin >= 4 && Cin <= 32; }

// What a *_scratch() entry answers: 0 for sizes <= 0 or a shape its entry refuses, else the formula, which is only evaluated then
#define AMS_ENTRY_SCRATCH(accepted, formula) ((accepted) ? ::ams::scratch_or_zero(formula) : (size_t)0)
static inline size_t scratch_or_zero(size_t need) { return need != (size_t)-1 ? need : 0; }

}  // namespace ams
