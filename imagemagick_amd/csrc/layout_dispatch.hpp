// Host-side helpers of the kernel launchers: the run-time pixel layout (Quantum type, channel
// count, alpha blending) turned into template arguments, the launch with more than 64 KB of dynamic
// LDS, the launch geometry of the pointwise streams, that of the one-thread-per-column operators and
// that of the operators that stage a window in LDS for 16 x 16 outputs.
#pragma once

#include "mh_internal.hpp"

#include <type_traits>

namespace mh {

// What f receives: `typename decltype(L)::Q`, `L.C` and `L.BLEND` are compile-time values.
template<typename Q_,int C_,bool BLEND_=false>
struct Layout
{
  using Q=Q_;
  static constexpr int C=C_;
  static constexpr bool BLEND=BLEND_;
};

// f(c) with the compile-time value c.value = channels; a channel count other than 1, 2 and 3 goes
// to 4.
template<class F>
static inline auto dispatch_channels(int channels,F &&f)
{
  switch (channels)
  {
    case 1: return f(std::integral_constant<int,1>{});
    case 2: return f(std::integral_constant<int,2>{});
    case 3: return f(std::integral_constant<int,3>{});
    default: return f(std::integral_constant<int,4>{});
  }
}

// f(q) with a value q of the Quantum type: uint16_t (MH_QUANTUM_U16) or float.
template<class F>
static inline auto dispatch_quantum(MhQuantumKind quantum,F &&f)
{
  return quantum == MH_QUANTUM_U16 ? f(uint16_t{}) : f(float{});
}

// f(Layout<Q,C>{}) with Q as above and C = channels, as above.
template<class F>
static inline auto dispatch_layout(MhQuantumKind quantum,int channels,F &&f)
{
  return dispatch_quantum(quantum,[&](auto q)
  {
    using Q=decltype(q);
    return dispatch_channels(channels,[&](auto c) { return f(Layout<Q,c.value>{}); });
  });
}

// ... for the kernels that exist for R,G,B[,A] frames only: f receives Layout<Q,3> or Layout<Q,4>
// and <Q,1>, <Q,2> are never instantiated.  The caller has rejected every other channel count.
template<class F>
static inline auto dispatch_colour_layout(MhQuantumKind quantum,int channels,F &&f)
{
  return dispatch_quantum(quantum,[&](auto q)
  {
    using Q=decltype(q);
    return channels == 3 ? f(Layout<Q,3>{}) : f(Layout<Q,4>{});
  });
}

// f(Layout<Q,C,BLEND>{}) for a Quantum type the caller has fixed, with BLEND = blend where the last
// channel can be an alpha (C = 2 or 4): <Q,1,true> and <Q,3,true> are never instantiated.
template<typename Q,class F>
static inline auto dispatch_channels_blend(int channels,bool blend,F &&f)
{
  return dispatch_channels(channels,[&](auto c)
  {
    if constexpr ((c.value == 2) || (c.value == 4))
      {
        if (blend)
          return f(Layout<Q,c.value,true>{});
      }
    return f(Layout<Q,c.value>{});
  });
}

// ... and with Q from the run-time Quantum kind
template<class F>
static inline auto dispatch_layout_blend(MhQuantumKind quantum,int channels,bool blend,F &&f)
{
  return dispatch_quantum(quantum,[&](auto q) { return dispatch_channels_blend<decltype(q)>(channels,blend,f); });
}

// ... for the kernels of four-channel frames only: f receives Layout<Q,4,false> or Layout<Q,4,true>
template<class F>
static inline auto dispatch_rgba_blend(MhQuantumKind quantum,bool blend,F &&f)
{
  return dispatch_quantum(quantum,[&](auto q)
  {
    using Q=decltype(q);
    return blend ? f(Layout<Q,4,true>{}) : f(Layout<Q,4,false>{});
  });
}

// ------------------------------------------------------------ dynamic LDS
// One launch and its check.  More than 64 KB of dynamic LDS needs the attribute (set per launch).
template<class... PARAMS,class... ARGS>
static MhStatus launch_dynamic_lds(void (*kernel)(PARAMS...),dim3 grid,dim3 block,size_t lds,hipStream_t stream,
  const ARGS &...args)
{
  if (lds > 64u*1024u)
    MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),hipFuncAttributeMaxDynamicSharedMemorySize,
      (int) lds));
  hipLaunchKernelGGL(kernel,grid,block,lds,stream,args...);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ------------------------------------------------------------ pointwise streams
// Pointwise kernels keep kPointBatch pixels per lane in flight: with one 8-byte load per lane
// the latency of the load -> (gather ->) compute -> store chain, not HBM, sets the rate
// (measured 1.2 TB/s for the Lab kernel before batching).
constexpr int kPointBatch=4;

static unsigned stream_grid(size_t npixels)
{
  size_t blocks=(npixels+255)/256;
  if (blocks > 8192)
    blocks=8192;
  if (blocks < 1)
    blocks=1;
  return (unsigned) blocks;
}

// ------------------------------------------------------------ one thread per column
// The operators of effects.hip: a thread per column (or per padded column, per column and colour channel, per sample
// of a flat array), kColumnBlock threads a block, a grid row per image row.
constexpr int kColumnBlock=256;

static inline dim3 column_grid(size_t columns,size_t rows=1)
{
  return dim3((unsigned) ((columns+kColumnBlock-1)/kColumnBlock),(unsigned) rows);
}

// ------------------------------------------------------------ 16 x 16 outputs per workgroup
// StatisticImage, the edge-preserving blurs and KuwaharaImage: a workgroup of kWindowBlock^2 threads
// stages the window of kWindowBlock x kWindowBlock outputs in LDS.
constexpr int kWindowBlock=16;

// MH_UNSUPPORTED when the frame does not fit the grid (or the kernels' int coordinates)
static inline MhStatus window_grid_check(const char *what,const View &src)
{
  if ((src.columns > 0x7fffffffu-kWindowBlock) || ((src.rows+kWindowBlock-1)/kWindowBlock > 65535u))
    return fail(MH_UNSUPPORTED,"%s: %zux%zu frame is outside the launch grid",what,src.columns,src.rows);
  return MH_OK;
}

static inline dim3 window_grid(int columns,int rows)
{
  return dim3((unsigned) ((columns+kWindowBlock-1)/kWindowBlock),(unsigned) ((rows+kWindowBlock-1)/kWindowBlock));
}

} // namespace mh
