// The launch layer of every tile launcher, of this directory and of the companion libraries: the encoder's
// dynamic LDS, the check that a kernel has no static LDS, the step from run-time choices to a kernel's template arguments, the
// launch itself and the 32-bit test of a decode's store side.  Host code; hgi_fused_impl.h includes it behind the tile procedure,
// whose geometry (buf_bytes, rbuf_bytes, NL) it names, and everything here is internal to the including unit.  How many tiles a
// decode keeps on a CU is hgi_launch_policy.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hgi_launch_policy.h"

namespace hgi {
namespace {

// ---- the encoder's LDS layout (k_enc_tiles'): the table at offset 0 (lut_at()), 256 bytes; `buf` behind it; `rbuf` behind
// that, from the next multiple of 16.  The three pointers stay spelled out in each kernel: taken from a function, whatever its
// form, the address arithmetic is folded in another order and the scheduler moves instructions of the kernels
// (profiles/r20_companion_kernels.md).
inline size_t enc_lds_bytes(int nh) { return (size_t)buf_bytes(nh) + ((rbuf_bytes(nh) + 15) & ~15) + 256; }

// The kernels address the quantizer's table from LDS offset 0 (lut_at()): only valid while the compiler placed no static LDS in
// front of the dynamic segment.  A build that breaks it fails here, on the host, not on the device.
inline hipError_t static_lds_is_empty(const void *kernel)
{
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, kernel);
    if (e != hipSuccess) return e;
    return fa.sharedSizeBytes == 0 ? hipSuccess : hipErrorInvalidDeviceFunction;
}

// One kernel, one wave per block, `blocks` of them: the static-LDS check, once per instantiation; then the launch and its error.
template <auto K, class... A>
hipError_t launch_tile_kernel(dim3 blocks, size_t lds, hipStream_t s, const A &...args)
{
    static const hipError_t lds0 = static_lds_is_empty(reinterpret_cast<const void *>(K));
    if (lds0 != hipSuccess) return lds0;
    hipLaunchKernelGGL(K, blocks, dim3(NL), lds, s, args...);
    return hipGetLastError();
}

// Run-time choices to template arguments: with_choices(f, OneOf<A...>{a}, OneOf<B...>{b}, ...) calls f(Const<a>{}, Const<b>{},
// ...), whose parameters a generic lambda can name as a kernel's template arguments.  A value that is none of its list ends
// the call with hipErrorInvalidValue.  Only the listed combinations are instantiated, in the order of the lists, the last
// choice running fastest -- and that is the order of the kernels in the unit's code object, which is not free: listed the
// other way round, typed encode's E = 4 kernels come out with other registers (profiles/r20_companion_kernels.md).
template <int V>
using Const = std::integral_constant<int, V>;
template <int... V>
struct OneOf {
    int v;
};

template <class F, int V, class... C>
hipError_t with_choices(const F &f, Const<V> c0, C... c)      // every choice made: they stand in the order given
{
    return f(c0, c...);
}

template <class F, int V0, int... V, class... C>
hipError_t with_choices(const F &f, OneOf<V0, V...> o, C... c)      // the first open choice moves behind the others as a constant
{
    if (o.v == V0) return with_choices(f, c..., Const<V0>{});
    if constexpr (sizeof...(V) > 0) return with_choices(f, OneOf<V...>{o.v}, c...);
    return hipErrorInvalidValue;
}

// Any interpolator but Crossed is LeftTop, as the kernels' INTERP has it
inline OneOf<kInterpCrossed, kInterpLeftTop> interp_choice(int interp)
{
    return {interp == kInterpCrossed ? kInterpCrossed : kInterpLeftTop};
}

// The store side of a decode into frames of `height` rows of `width` bytes, `out_pitch` apart: whether one frame is addressed
// with 32 bits, and then its pitch and span (a one-row frame never steps by the pitch).
struct StoreSide {
    uint64_t pitch, span;
    bool ok;
};

inline StoreSide store_side_32(uint32_t height, uint32_t width, uint64_t out_pitch)
{
    StoreSide t;
    t.pitch = height > 1 ? out_pitch : width;
    t.span = (uint64_t)(height - 1) * t.pitch + width;
    t.ok = height == 1 || (t.pitch < (1ull << 32) && t.span + 64 < (1ull << 32));
    return t;
}

}  // namespace
}  // namespace hgi
