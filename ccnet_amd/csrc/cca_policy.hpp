// cca_policy.hpp -- the 16-byte buffer primitives of cca_platform.hpp with a compile-time CACHE POLICY (option "stream_policy",
// cca_api.hip).  The policy changes where a line is kept on its way through L2 and the Infinity Cache and nothing
// else: the instruction count, the wait counts and every result bit of a kernel are those of its default-policy instantiation.
//   CP_DEFAULT  the access as cca_platform.hpp issues it
//   CP_NT       non-temporal ("nt"): a last use, or an output nobody reads again -- the line does not compete for residency
//   CP_WT       write-through ("sc1"), 16-BYTE STORES ONLY: the line leaves L2 as it is written instead of staying dirty until the
//               kernel boundary writes it back (MI355X: narrower write-through stores cost 2.7x - 6x per byte, so the 4- and
//               8-byte stores of the library keep the default)
// On the builtins the policy is the ``aux`` operand, in the asm statement of the uncounted LDS-DMA it is the modifier.
// Under the SIMT emulator of the CPU tests (recognised by CCA_EMU_SITE, which only its cca_platform.hpp defines) a policy has
// no meaning: the variants forward to the plain primitives and hand the call site on, so its diagnostics name the kernel line.
#pragma once
#include <cca_platform.hpp>      // (angle form, as cca_common.hpp: the CPU tests put their own header of that name first)

namespace cca {

constexpr int CP_DEFAULT = 0, CP_NT = 2, CP_WT = 16;

// A kernel's policy (its last template parameter): which of its operand classes carry a non-default policy.
//   SP_FEAT_NT   the feature tiles (LDS-DMA ring / double-buffer fills)      SP_ADD_NT  the addend (the column partial)
//   SP_SRC_NT    the residual of an NCHW epilogue / the source of a transposing pass
//   SP_ST_NT, SP_ST_WT   the 16-byte stores of the kernel's output (one of the two)
constexpr int SP_FEAT_NT = 1, SP_ADD_NT = 2, SP_SRC_NT = 4, SP_ST_NT = 8, SP_ST_WT = 16;
constexpr int sp_load(int pol, int bit) { return (pol & bit) ? CP_NT : CP_DEFAULT; }
constexpr int sp_store(int pol) { return (pol & SP_ST_WT) ? CP_WT : (pol & SP_ST_NT) ? CP_NT : CP_DEFAULT; }

#ifdef CCA_EMU_SITE
template <int CP>
__device__ inline f32x4 fbuf_load_x4_cp(const FBuf &b, int voff_bytes, int soff_bytes, CCA_EMU_SITE) {
    return fbuf_load_x4(b, voff_bytes, soff_bytes, site, site_file);
}
template <int CP>
__device__ inline void fbuf_store_x4_cp(const FBuf &b, f32x4 v, int voff_bytes, int soff_bytes, CCA_EMU_SITE) {
    fbuf_store_x4(b, v, voff_bytes, soff_bytes, site, site_file);
}
template <int CP>
__device__ inline void fbuf_store_x2_cp(const FBuf &b, uint32_t v0, uint32_t v1, int voff_bytes, int soff_bytes, CCA_EMU_SITE) {
    fbuf_store_x2(b, v0, v1, voff_bytes, soff_bytes, site, site_file);
}
template <int CP>
__device__ inline void fbuf_load_to_lds_x4_uncounted_cp(const FBuf &b, float *lds_wave_base, int voff_bytes, CCA_EMU_SITE) {
    fbuf_load_to_lds_x4_uncounted(b, lds_wave_base, voff_bytes, site, site_file);
}
#else
template <int CP>
__device__ __forceinline__ f32x4 fbuf_load_x4_cp(const FBuf &b, int voff_bytes, int soff_bytes) {
    static_assert(CP == CP_DEFAULT || CP == CP_NT, "loads: default or nt");
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b, voff_bytes, soff_bytes, CP));
}
template <int CP>
__device__ __forceinline__ void fbuf_store_x4_cp(const FBuf &b, f32x4 v, int voff_bytes, int soff_bytes) {
    static_assert(CP == CP_DEFAULT || CP == CP_NT || CP == CP_WT, "16-byte stores: default, nt or write-through");
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), b, voff_bytes, soff_bytes, CP);
}
template <int CP>
__device__ __forceinline__ void fbuf_store_x2_cp(const FBuf &b, uint32_t v0, uint32_t v1, int voff_bytes, int soff_bytes) {
    static_assert(CP == CP_DEFAULT || CP == CP_NT, "8-byte stores: default or nt (write-through is offered at 16 bytes only)");
    __builtin_amdgcn_raw_buffer_store_b64(u32x2s{v0, v1}, b, voff_bytes, soff_bytes, CP);
}
// (the statement of cca_platform.hpp with the modifier in front of ``lds``; M0 saved and restored as there)
template <int CP>
__device__ __forceinline__ void fbuf_load_to_lds_x4_uncounted_cp(const FBuf &b, float *lds_wave_base, int voff_bytes) {
    static_assert(CP == CP_DEFAULT || CP == CP_NT, "loads: default or nt");
    if constexpr (CP == CP_DEFAULT) {
        fbuf_load_to_lds_x4_uncounted(b, lds_wave_base, voff_bytes);
    } else {
        const unsigned lds_addr = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)lds_wave_base);
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen nt lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff_bytes), "s"(lds_addr), "s"(b) : "memory");
    }
}
#endif

}  // namespace cca
