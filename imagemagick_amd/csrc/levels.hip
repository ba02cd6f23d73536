// The tone-curve ("level") operators of MagickCore/enhance.c, evaluated per sample in fp64 in the
// reference's operation order (no contraction), and the range scan under MinMaxStretchImage.
//
//   LevelImage :2913-3018       ClampToQuantum(QuantumRange*gamma_pow(scale*(q-black),1/gamma)), then
//                               ClampImage (threshold.c:1087: on float Quantum the stored float is
//                               clamped with ClampPixel), fused here: round to Quantum, then clamp
//   LevelizeImage :3062-3170    ClampToQuantum(gamma_pow(QuantumScale*q,gamma)*(white-black)+black)
//   NegateImage :3940-4100      QuantumRange-q in the Quantum's own arithmetic; with `grayscale`
//                               only pixels that IsPixelGray (pixel-accessor.h:561-578)
//   SigmoidalContrastImage :4267-4407   tanh form (MAGICKCORE_HAVE_ATANH); Sigmoidal(a,b,0) and
//                               Sigmoidal(a,b,1) are formed on the host and passed in; float samples at the
//                               curve's zero are the host's (LevelsDoubt, mh_internal.hpp)
//   GetImageRange statistic.c:1851-1929   per channel minimum and maximum, and those of column 0 of
//                               channel 0 (every row is seeded with p[0], whatever the mask)
//
// On Q16 the curves that call libm (gamma != 1, the sigmoidals, GammaImage) are tabulated on the
// host with the libm the reference links and applied by launch_apply_lut; the kernels here serve Q16
// where no libm is involved, and float Quantum always (the device's pow / tanh / atanh: one float
// ULP).  There is no FAST variant.
//
// MI355X mapping:
//   levels_point_kernel   one lane per pixel, one vector load and one vector store, grid-stride; the
//                         mode is uniform over the grid and selected outside the pixel loop
//   levels_range_kernel   one read pass: per-lane registers, a wave reduction by shuffles, one LDS
//                         stage per workgroup, per-workgroup partials
//   levels_range_finish_kernel   one workgroup folds the partials; minimum and maximum do not depend
//                         on the order, so any tree gives the reference's bits
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"

#include <algorithm>
#include <cfloat>

namespace mh {

constexpr int kLevelsThreads=256;
constexpr int kLevelsWaves=kLevelsThreads/64;
constexpr unsigned kLevelsRangeMaxBlocks=1024;
constexpr int kRangeSlots=2*(MH_MAX_CHANNELS+1);     // [2c] minimum, [2c+1] maximum; c = MH_MAX_CHANNELS: column 0 of channel 0

static unsigned levels_grid(size_t npixels,unsigned most)
{
  size_t blocks=(npixels+kLevelsThreads-1)/kLevelsThreads;
  if (blocks > most)
    blocks=most;
  if (blocks < 1)
    blocks=1;
  return (unsigned) blocks;
}

struct LevelsPointArgs
{
  void *pixels;
  unsigned long long count;            // pixels
  LevelsParams p;
};

// gamma_pow, enhance.c:2317-2320
static __device__ __forceinline__ double gamma_pow(double value,double gamma)
{
  return value < 0.0 ? value : pow(value,gamma);
}

// ClampPixel on the stored Quantum (ClampImage, threshold.c:1163); a Q16 sample is in range already
template<typename Q>
static __device__ __forceinline__ Q clamp_stored(Q q)
{
  if constexpr (QuantumOps<Q>::is_float)
    {
      if ((double) q < 0.0)
        return 0.0f;
      if ((double) q >= kQR)
        return 65535.0f;
    }
  return q;
}

template<typename Q,int MODE>
static __device__ __forceinline__ Q levels_sample(const LevelsParams &p,Q q)
{
  const double pixel=(double) q;
  if constexpr (MODE == MH_LEVELS_LEVEL)
    {
      // pow(v,1.0) is v: gamma == 1 needs no libm
      const double v=p.a*(pixel-p.b);
      return clamp_stored<Q>(QuantumOps<Q>::clamp(kQR*v));
    }
  else if constexpr (MODE == MH_LEVELS_LEVEL_POW)
    return clamp_stored<Q>(QuantumOps<Q>::clamp(kQR*gamma_pow(p.a*(pixel-p.b),p.c)));
  else if constexpr (MODE == MH_LEVELS_LEVELIZE)
    return QuantumOps<Q>::clamp((kQS*pixel)*p.a+p.b);
  else if constexpr (MODE == MH_LEVELS_LEVELIZE_POW)
    return QuantumOps<Q>::clamp(gamma_pow(kQS*pixel,p.c)*p.a+p.b);
  else if constexpr (MODE == MH_LEVELS_SIGMOIDAL)
    {
      // ScaledSigmoidal, enhance.c:4207, :4228-4230: p.a = 0.5*contrast, p.b = QuantumScale*midpoint,
      // p.c = Sigmoidal(0), p.d = Sigmoidal(1)
      // (a sample of exactly 0 is Sigmoidal(0) itself: the host's value, so the difference is the reference's 0)
      const double s=pixel == 0.0 ? p.c : tanh(p.a*(kQS*pixel-p.b));
      return QuantumOps<Q>::clamp(kQR*((s-p.c)/(p.d-p.c)));
    }
  else if constexpr (MODE == MH_LEVELS_SIGMOIDAL_INVERSE)
    {
      // InverseScaledSigmoidal, enhance.c:4240-4256: p.a = 2.0/contrast
      const double argument=(p.d-p.c)*(kQS*pixel)+p.c;
      const double clamped=argument < -1+kEps ? -1+kEps : (argument > 1-kEps ? 1-kEps : argument);
      // (a sample of exactly 0: the argument is p.c, and p.e the host's atanh of it)
      return QuantumOps<Q>::clamp(kQR*(p.b+p.a*(pixel == 0.0 ? p.e : atanh(clamped))));
    }
  else
    {
      // QuantumRange-q in Quantum arithmetic, enhance.c:4025, :4088
      if constexpr (QuantumOps<Q>::is_float)
        return 65535.0f-q;
      else
        return (Q) (65535u-(unsigned) q);
    }
}

// IsPixelGray, pixel-accessor.h:561-578; with fewer than three colour channels green and blue read
// offset 0 (the channel map's zeroed entries) and every pixel is gray
template<typename Q,int C>
static __device__ __forceinline__ bool levels_pixel_gray(const Q (&q)[C],int colours)
{
  if constexpr (C < 3)
    return true;
  else
    {
      if (colours < 3)
        return true;
      const double red_green=(double) q[0]-(double) q[1],green_blue=(double) q[1]-(double) q[2];
      return (fabs(red_green) < kEps) && (fabs(green_blue) < kEps);
    }
}

// a sample the host evaluates: not 0 (that one is exact), below p.doubt in magnitude (a NaN is not)
template<typename Q>
static __device__ __forceinline__ bool levels_doubtful(const LevelsParams &p,Q q)
{
  const double v=(double) q;
  return (v != 0.0) && (fabs(v) < p.doubt);
}

template<typename Q,int C,int MODE>
static __device__ __forceinline__ void levels_point_loop(const LevelsPointArgs &a)
{
  Q *pixels=static_cast<Q *>(a.pixels);
  const unsigned long long stride=(unsigned long long) gridDim.x*kLevelsThreads;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kLevelsThreads+threadIdx.x; i < a.count; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
      if constexpr (MODE == MH_LEVELS_NEGATE_GRAY)
        if (!levels_pixel_gray<Q,C>(q,a.p.colours))
          continue;
#pragma unroll
      for (int c=0; c < C; c++)
        if (((a.p.update_mask >> c) & 1u) != 0)
          {
            if constexpr (QuantumOps<Q>::is_float && ((MODE == MH_LEVELS_SIGMOIDAL) || (MODE == MH_LEVELS_SIGMOIDAL_INVERSE)))
              if ((a.p.doubt_list != nullptr) && levels_doubtful(a.p,q[c]))
                {
                  // the host's libm decides this one (launch_levels_scatter); what is stored below is overwritten
                  const unsigned long long slot=atomicAdd(a.p.doubt_count,1ull);
                  if (slot < a.p.doubt_capacity)
                    {
                      a.p.doubt_list[slot].index=i*C+(unsigned long long) c;
                      a.p.doubt_list[slot].original=(float) q[c];
                    }
                }
            q[c]=levels_sample<Q,MODE>(a.p,q[c]);
          }
      store_pixel<Q,C>(pixels+i*C,q);
    }
}

// the doubtful samples of a float frame under a sigmoidal, counted before the point kernel records them
template<typename Q,int C>
__global__ __launch_bounds__(kLevelsThreads)
void levels_doubt_count_kernel(LevelsPointArgs a)
{
  const Q *pixels=static_cast<const Q *>(a.pixels);
  const unsigned long long stride=(unsigned long long) gridDim.x*kLevelsThreads;
  unsigned long long n=0;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kLevelsThreads+threadIdx.x; i < a.count; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
#pragma unroll
      for (int c=0; c < C; c++)
        if ((((a.p.update_mask >> c) & 1u) != 0) && levels_doubtful(a.p,q[c]))
          n++;
    }
  if (n != 0)
    atomicAdd(a.p.doubt_count,n);
}

// the host's values of the doubtful samples, each to its place
template<typename Q>
__global__ __launch_bounds__(kLevelsThreads)
void levels_scatter_kernel(Q *pixels,unsigned long long samples,const LevelsDoubt *list,unsigned long long count)
{
  const unsigned long long stride=(unsigned long long) gridDim.x*kLevelsThreads;
  for (unsigned long long k=(unsigned long long) blockIdx.x*kLevelsThreads+threadIdx.x; k < count; k+=stride)
    if (list[k].index < samples)
      pixels[list[k].index]=(Q) list[k].value;
}

template<typename Q,int C>
__global__ __launch_bounds__(kLevelsThreads)
void levels_point_kernel(LevelsPointArgs a)
{
  switch (a.p.mode)
  {
    case MH_LEVELS_LEVEL: levels_point_loop<Q,C,MH_LEVELS_LEVEL>(a); break;
    case MH_LEVELS_LEVEL_POW: levels_point_loop<Q,C,MH_LEVELS_LEVEL_POW>(a); break;
    case MH_LEVELS_LEVELIZE: levels_point_loop<Q,C,MH_LEVELS_LEVELIZE>(a); break;
    case MH_LEVELS_LEVELIZE_POW: levels_point_loop<Q,C,MH_LEVELS_LEVELIZE_POW>(a); break;
    case MH_LEVELS_SIGMOIDAL: levels_point_loop<Q,C,MH_LEVELS_SIGMOIDAL>(a); break;
    case MH_LEVELS_SIGMOIDAL_INVERSE: levels_point_loop<Q,C,MH_LEVELS_SIGMOIDAL_INVERSE>(a); break;
    case MH_LEVELS_NEGATE: levels_point_loop<Q,C,MH_LEVELS_NEGATE>(a); break;
    default: levels_point_loop<Q,C,MH_LEVELS_NEGATE_GRAY>(a); break;
  }
}

// ------------------------------------------------------------------ range
struct LevelsRangeArgs
{
  const void *pixels;
  unsigned long long count;            // pixels; 0: only column 0 of channel 0 is scanned
  unsigned long long columns,rows;
  double *partials;                    // [blocks][kRangeSlots]
  unsigned blocks;
  double *result;                      // [kRangeSlots]
};

// slot k of every lane folded over the workgroup; thread 0 holds the result
static __device__ __forceinline__ double levels_fold(double v,bool maximum,double *stage)
{
#pragma unroll
  for (int offset=32; offset > 0; offset>>=1)
    {
      const double other=__shfl_down(v,offset,64);
      v=maximum ? (other > v ? other : v) : (other < v ? other : v);
    }
  const int lane=(int) (threadIdx.x & 63),wave=(int) (threadIdx.x >> 6);
  __syncthreads();                     // the previous slot's stage has been read
  if (lane == 0)
    stage[wave]=v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w=1; w < kLevelsWaves; w++)
      v=maximum ? (stage[w] > v ? stage[w] : v) : (stage[w] < v ? stage[w] : v);
  return v;
}

template<typename Q,int C>
__global__ __launch_bounds__(kLevelsThreads)
void levels_range_kernel(LevelsRangeArgs a)
{
  __shared__ double stage[kLevelsWaves];
  const Q *pixels=static_cast<const Q *>(a.pixels);
  double low[C+1],high[C+1];
#pragma unroll
  for (int c=0; c <= C; c++)
    {
      low[c]=DBL_MAX;
      high[c]=-DBL_MAX;
    }
  const unsigned long long stride=(unsigned long long) gridDim.x*kLevelsThreads;
  const unsigned long long first=(unsigned long long) blockIdx.x*kLevelsThreads+threadIdx.x;
  for (unsigned long long i=first; i < a.count; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
#pragma unroll
      for (int c=0; c < C; c++)
        {
          const double v=(double) q[c];
          low[c]=v < low[c] ? v : low[c];
          high[c]=v > high[c] ? v : high[c];
        }
    }
  // the seed of every row: the offset-0 sample of its first pixel
  for (unsigned long long y=first; y < a.rows; y+=stride)
    {
      const double v=(double) pixels[y*a.columns*C];
      low[C]=v < low[C] ? v : low[C];
      high[C]=v > high[C] ? v : high[C];
    }
  double *out=a.partials+(size_t) blockIdx.x*kRangeSlots;
#pragma unroll
  for (int c=0; c <= C; c++)
    {
      const int slot=c == C ? MH_MAX_CHANNELS : c;
      const double l=levels_fold(low[c],false,stage),h=levels_fold(high[c],true,stage);
      if (threadIdx.x == 0)
        {
          out[2*slot]=l;
          out[2*slot+1]=h;
        }
    }
  if constexpr (C < MH_MAX_CHANNELS)
    if (threadIdx.x == 0)
      for (int c=C; c < MH_MAX_CHANNELS; c++)
        {
          out[2*c]=DBL_MAX;
          out[2*c+1]=-DBL_MAX;
        }
}

__global__ __launch_bounds__(kLevelsThreads)
void levels_range_finish_kernel(LevelsRangeArgs a)
{
  __shared__ double stage[kLevelsWaves];
  for (int slot=0; slot < kRangeSlots; slot++)
    {
      const bool maximum=(slot & 1) != 0;
      double v=maximum ? -DBL_MAX : DBL_MAX;
      for (unsigned b=threadIdx.x; b < a.blocks; b+=kLevelsThreads)
        {
          const double other=a.partials[(size_t) b*kRangeSlots+slot];
          v=maximum ? (other > v ? other : v) : (other < v ? other : v);
        }
      v=levels_fold(v,maximum,stage);
      if (threadIdx.x == 0)
        a.result[slot]=v;
    }
}

// ------------------------------------------------------------------ launchers
MhStatus launch_levels_point(const View &img,const LevelsParams &params)
{
  if ((img.columns == 0) || (img.rows == 0) || (params.update_mask == 0))
    return MH_OK;
  LevelsPointArgs a={};
  a.pixels=img.pixels;
  a.count=(unsigned long long) img.columns*(unsigned long long) img.rows;
  a.p=params;
  static const char *const names[]={"levels_level","levels_level_pow","levels_levelize","levels_levelize_pow",
    "levels_sigmoidal","levels_sigmoidal_inverse","levels_negate","levels_negate_gray"};
  if ((params.mode < 0) || (params.mode > MH_LEVELS_NEGATE_GRAY))
    return fail(MH_BAD_ARGUMENT,"levels: unknown mode %d",params.mode);
  const unsigned blocks=levels_grid((size_t) a.count,8192u);
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    ProfileScope prof(names[params.mode],img.stream);
    hipLaunchKernelGGL((levels_point_kernel<typename decltype(L)::Q,L.C>),dim3(blocks),dim3(kLevelsThreads),0,
      img.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

MhStatus launch_levels_doubt_count(const View &img,const LevelsParams &params,unsigned long long *count_device)
{
  LevelsPointArgs a={};
  a.pixels=img.pixels;
  a.count=(unsigned long long) img.columns*(unsigned long long) img.rows;
  a.p=params;
  a.p.doubt_count=count_device;
  const unsigned blocks=levels_grid((size_t) a.count,kLevelsRangeMaxBlocks);
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    ProfileScope prof("levels_doubt_count",img.stream);
    hipLaunchKernelGGL((levels_doubt_count_kernel<typename decltype(L)::Q,L.C>),dim3(blocks),dim3(kLevelsThreads),0,
      img.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

MhStatus launch_levels_scatter(const View &img,const LevelsDoubt *list,unsigned long long count)
{
  if (count == 0)
    return MH_OK;
  if (img.quantum != MH_QUANTUM_F32)
    return fail(MH_BAD_ARGUMENT,"levels: only a float frame has doubtful samples");
  const unsigned long long samples=(unsigned long long) img.columns*(unsigned long long) img.rows*
    (unsigned long long) img.channels;
  ProfileScope prof("levels_scatter",img.stream);
  hipLaunchKernelGGL((levels_scatter_kernel<float>),dim3(levels_grid((size_t) count,1024u)),dim3(kLevelsThreads),0,
    img.stream,static_cast<float *>(img.pixels),samples,list,count);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_levels_range(const View &img,bool column0_only,double *result_device)
{
  LevelsRangeArgs a={};
  a.pixels=img.pixels;
  a.columns=img.columns;
  a.rows=img.rows;
  a.count=column0_only ? 0ull : (unsigned long long) img.columns*(unsigned long long) img.rows;
  if ((img.columns == 0) || (img.rows == 0))
    a.rows=a.count=0;
  a.blocks=levels_grid(column0_only ? img.rows : (size_t) a.count,kLevelsRangeMaxBlocks);
  Temp partials;
  MH_TRY(partials.alloc(img.device,(size_t) a.blocks*kRangeSlots*sizeof(double),img.stream));
  a.partials=partials.as<double>();
  a.result=result_device;
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    ProfileScope prof("levels_range",img.stream);
    hipLaunchKernelGGL((levels_range_kernel<typename decltype(L)::Q,L.C>),dim3(a.blocks),dim3(kLevelsThreads),0,
      img.stream,a);
    MH_HIP(hipGetLastError());
    hipLaunchKernelGGL(levels_range_finish_kernel,dim3(1),dim3(kLevelsThreads),0,img.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

} // namespace mh
