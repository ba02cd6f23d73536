// Histogram operators: the histogram kernels (global atomics, LDS-privatised, packed 16-bit counters), the fused
// FAST sRGB -> Lab + histogram kernel and ContrastStretchImage's levels straight from its slabs, the on-device LUT
// build, the LUT-apply kernels and the float EqualizeImage map.
//
// Reference semantics restated from:
//   GetPixelIntensity                      MagickCore/pixel.c:2356-2455
//   histogram / LUT apply                  MagickCore/enhance.c:1616-1647, :1778-1788, :2102-2133, :2252-2262
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "pixel_intensity.hpp"
#include "colour_math.hpp"

namespace mh {

// ---------------------------------------------------------------- histogram
// 65536 bins x C channels of 64-bit counts (0.5-2 MiB) do not fit LDS, so the
// counts live in global memory (L2 / Infinity-Cache resident) and are updated
// with device-scope atomics.  Two things keep the atomic traffic down:
//   * in intensity mode every channel bins the same value, so only channel 0
//     is accumulated and a 65536-element kernel replicates it afterwards;
//   * when neighbouring lanes agree on the bin (smooth images, 8-bit data) the
//     wave folds equal bins first and issues one atomic per distinct bin.
static __device__ __forceinline__ void histogram_add(unsigned long long *counts,unsigned bin,
  int stride,int c,bool valid)
{
  const int lane=(int) (threadIdx.x & 63);
  unsigned neighbour=__shfl(bin,(lane+1) & 63,64);
  unsigned long long agree=__ballot(valid && (neighbour == bin));
  if (__popcll(agree) < 16)
    {
      if (valid)
        atomicAdd(counts+(size_t) bin*stride+c,1ull);
      return;
    }
  // match-any by leader election over the still-unserved lanes
  unsigned long long remaining=__ballot(valid);
  while (remaining != 0)
    {
      int leader=__ffsll((long long) remaining)-1;
      unsigned leader_bin=__shfl(bin,leader,64);
      unsigned long long same=__ballot(valid && (bin == leader_bin)) & remaining;
      if (lane == leader)
        atomicAdd(counts+(size_t) leader_bin*stride+c,(unsigned long long) __popcll(same));
      remaining&=~same;
    }
}

template<typename Q,int C>
__global__ __launch_bounds__(256)
void histogram_kernel(const Q *pixels,size_t npixels,int intensity_mode,IntensityParams ip,
  unsigned long long *counts)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  const size_t rounds=(npixels+stride-1)/stride;
  size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x;
  for (size_t k=0; k < rounds; k++,i+=stride)
    {
      const bool valid=i < npixels;
      Q q[C];
      load_pixel<Q,C>(pixels+(valid ? i : 0)*C,q);
      if (intensity_mode)
        {
          // ScaleQuantumToMap(ClampToQuantum(intensity)): every channel bins the same value
          unsigned bin=QuantumOps<Q>::map_index(QuantumOps<Q>::clamp(pixel_intensity<Q,C>(q,ip)));
          histogram_add(counts,bin,C,0,valid);
        }
      else
        {
#pragma unroll
          for (int c=0; c < C; c++)
            {
              unsigned bin=QuantumOps<Q>::map_index(QuantumOps<Q>::clamp((double) q[c]));
              histogram_add(counts,bin,C,c,valid);
            }
        }
    }
}

// intensity mode: channel 0 holds this call's counts (added on top of what the
// caller passed in); propagate the increment to the other channels
__global__ __launch_bounds__(256)
void histogram_replicate_kernel(unsigned long long *counts,const unsigned long long *before,int channels)
{
  unsigned bin=blockIdx.x*blockDim.x+threadIdx.x;
  if (bin > 65535u)
    return;
  unsigned long long delta=counts[(size_t) bin*channels]-before[bin];
  for (int c=1; c < channels; c++)
    counts[(size_t) bin*channels+c]+=delta;
}

__global__ __launch_bounds__(256)
void histogram_snapshot_kernel(const unsigned long long *counts,unsigned long long *before,int channels)
{
  unsigned bin=blockIdx.x*blockDim.x+threadIdx.x;
  if (bin <= 65535u)
    before[bin]=counts[(size_t) bin*channels];
}

// Intensity mode, LDS-privatised.  65 536 bins do not fit LDS as 32-bit counters
// (256 KB > 160 KB), so a persistent workgroup (one per CU, 1024 threads) bins its
// slice of the image twice — bins 0..32767, then 32768..65535 — into a 128 KB LDS
// table with ds_add (no global atomics: on uniform-random Q16 data the global-atomic
// kernel above is bound by 16.7 M L2 atomics per 4096^2 image), and writes each
// half to its own slab; a small kernel sums the slabs into the caller's table
// (all channels of a bin receive the same count in this mode).  The second read
// of the slice comes from L2 / Infinity Cache.
constexpr int kHistHalf=32768;

template<typename Q,int C>
__global__ __launch_bounds__(1024)
void histogram_lds_kernel(const Q *pixels,size_t npixels,IntensityParams ip,unsigned *slabs)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned *table=reinterpret_cast<unsigned *>(smem_raw);
  const size_t per=(npixels+gridDim.x-1)/gridDim.x;
  const size_t begin=(size_t) blockIdx.x*per;
  size_t end=begin+per;
  end=end < npixels ? end : npixels;
  for (int half=0; half < 2; half++)
    {
      for (int i=(int) threadIdx.x; i < kHistHalf; i+=1024)
        table[i]=0u;
      __syncthreads();
      const unsigned base=(unsigned) half*kHistHalf;
      constexpr int BATCH=4;
      for (size_t i0=begin+threadIdx.x; i0 < end; i0+=(size_t) 1024*BATCH)
        {
          Q q[BATCH][C];
#pragma unroll
          for (int k=0; k < BATCH; k++)
            {
              size_t i=i0+(size_t) 1024*k;
              load_pixel<Q,C>(pixels+(i < end ? i : end-1)*C,q[k]);
            }
#pragma unroll
          for (int k=0; k < BATCH; k++)
            if (i0+(size_t) 1024*k < end)
              {
                unsigned bin=QuantumOps<Q>::map_index(QuantumOps<Q>::clamp(pixel_intensity<Q,C>(q[k],ip)));
                unsigned local=bin-base;
                if (local < (unsigned) kHistHalf)
                  atomicAdd(table+local,1u);
              }
        }
      __syncthreads();
      unsigned *slab=slabs+((size_t) blockIdx.x*2+half)*kHistHalf;
      for (int i=(int) threadIdx.x; i < kHistHalf; i+=1024)
        slab[i]=table[i];
      __syncthreads();
    }
}

// grid (256, kSlabGroups): block y sums its share of the per-workgroup slabs for 256 bins
// and adds the partial sum to the caller's table (one 64-bit atomic per bin and channel,
// kSlabGroups-way contention at most) — 8x the loads in flight of a single pass per bin.
constexpr int kSlabGroups=8;

__global__ __launch_bounds__(256)
void histogram_slab_reduce_kernel(const unsigned *slabs,int nblocks,unsigned long long *counts,int channels)
{
  const unsigned bin=blockIdx.x*blockDim.x+threadIdx.x;
  if (bin > 65535u)
    return;
  const unsigned half=bin/kHistHalf,local=bin%kHistHalf;
  const int per=(nblocks+kSlabGroups-1)/kSlabGroups;
  const int b0=(int) blockIdx.y*per;
  const int b1=b0+per < nblocks ? b0+per : nblocks;
  unsigned long long sum=0;
#pragma unroll 8
  for (int b=b0; b < b1; b++)
    sum+=slabs[((size_t) b*2+half)*kHistHalf+local];
  if (sum != 0)
    for (int c=0; c < channels; c++)
      atomicAdd(counts+(size_t) bin*channels+c,sum);
}

template<typename Q,int C>
static MhStatus histogram_intensity_lds(const View &src,const IntensityParams &ip,unsigned long long *hist)
{
  const size_t n=src.columns*src.rows;
  const int nblocks=compute_units(src.device);
  Temp slabs;
  MH_TRY(slabs.alloc(src.device,(size_t) nblocks*2*kHistHalf*sizeof(unsigned),src.stream));
  const size_t lds=(size_t) kHistHalf*sizeof(unsigned);
  MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&histogram_lds_kernel<Q,C>),
    hipFuncAttributeMaxDynamicSharedMemorySize,(int) lds));
  {
    ProfileScope prof("histogram",src.stream);
    hipLaunchKernelGGL((histogram_lds_kernel<Q,C>),dim3(nblocks),dim3(1024),lds,src.stream,
      static_cast<const Q *>(src.pixels),n,ip,slabs.as<unsigned>());
    hipLaunchKernelGGL(histogram_slab_reduce_kernel,dim3(256,kSlabGroups),dim3(256),0,src.stream,
      slabs.as<unsigned>(),nblocks,hist,C);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// Intensity mode on Q16, one pass: 65 536 sixteen-bit counters DO fit (128 KB), two to a
// 32-bit LDS word, incremented with ds_add_u32 of 1 or 1<<16.  A workgroup bins at most 65 534
// pixels into its table, so no counter can wrap into its neighbour; the handful of pixels of an
// over-full share go straight to the caller's table with global atomics.  Each workgroup then
// writes its packed table (128 KB) to its slab and histogram_packed_reduce_kernel sums the slabs:
// the frame is read once, against twice by the 32-bit half-range kernel below.
constexpr unsigned kPackedCapacity=65534u;     // even: the RGBA path loads pixel pairs

// the shared tail of the packed-table kernels: LDS table -> the workgroup's slab
static __device__ __forceinline__ void packed_table_to_slab(const unsigned *table,unsigned *slabs)
{
  uint4 *slab=reinterpret_cast<uint4 *>(slabs+(size_t) blockIdx.x*32768);
  const uint4 *packed=reinterpret_cast<const uint4 *>(table);
  for (int i=(int) threadIdx.x; i < 8192; i+=1024)
    slab[i]=packed[i];
}

template<typename Q,int C,bool PLAIN>
__global__ __launch_bounds__(1024)
void histogram_packed_kernel(const Q *pixels,size_t npixels,IntensityParams ip,unsigned *slabs,
  unsigned long long *counts,int wide)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned *table=reinterpret_cast<unsigned *>(smem_raw);
  for (int i=(int) threadIdx.x; i < 32768; i+=1024)
    table[i]=0u;
  __syncthreads();
  size_t per=(npixels+gridDim.x-1)/gridDim.x;
  per+=per & 1;                                // shares start on a pixel pair
  size_t begin=(size_t) blockIdx.x*per;
  begin=begin < npixels ? begin : npixels;
  size_t end=begin+per;
  end=end < npixels ? end : npixels;
  const size_t packed_end=end-begin > kPackedCapacity ? begin+kPackedCapacity : end;
  auto count=[&](const Q (&q)[C])
  {
    const unsigned bin=QuantumOps<Q>::map_index(QuantumOps<Q>::clamp(pixel_intensity_of<PLAIN,Q,C>(q,ip)));
    atomicAdd(table+(bin >> 1),(bin & 1u) != 0u ? 0x10000u : 1u);
  };
  size_t done=begin;                           // pixels [begin, done) are in the LDS table
  if constexpr ((C == 4) && (sizeof(Q) == 2))
    if (wide != 0)
      {
        // 16-byte loads: two RGBA pixels per lane, eight loads in flight
        constexpr int BATCH=8;
        const uint4 *pairs=reinterpret_cast<const uint4 *>(pixels)+begin/2;
        const size_t npairs=(packed_end-begin)/2;
        for (size_t i0=threadIdx.x; i0 < npairs; i0+=(size_t) 1024*BATCH)
          {
            uint4 v[BATCH];
#pragma unroll
            for (int k=0; k < BATCH; k++)
              {
                const size_t i=i0+(size_t) 1024*k;
                v[k]=pairs[i < npairs ? i : npairs-1];
              }
#pragma unroll
            for (int k=0; k < BATCH; k++)
              if (i0+(size_t) 1024*k < npairs)
                {
                  const uint16_t a[4]={(uint16_t) v[k].x,(uint16_t) (v[k].x >> 16),(uint16_t) v[k].y,(uint16_t) (v[k].y >> 16)};
                  const uint16_t b[4]={(uint16_t) v[k].z,(uint16_t) (v[k].z >> 16),(uint16_t) v[k].w,(uint16_t) (v[k].w >> 16)};
                  count(a);
                  count(b);
                }
          }
        done=begin+2*npairs;
      }
  constexpr int BATCH=4;
  for (size_t i0=done+threadIdx.x; i0 < end; i0+=(size_t) 1024*BATCH)
    {
      Q q[BATCH][C];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) 1024*k;
          load_pixel<Q,C>(pixels+(i < end ? i : end-1)*C,q[k]);
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) 1024*k;
          if (i >= end)
            continue;
          if (i < packed_end)
            count(q[k]);
          else
            {
              // beyond what the 16-bit counters may hold: the caller's table directly
              const unsigned bin=QuantumOps<Q>::map_index(QuantumOps<Q>::clamp(pixel_intensity_of<PLAIN,Q,C>(q[k],ip)));
              for (int c=0; c < C; c++)
                atomicAdd(counts+(size_t) bin*C+c,1ull);
            }
        }
    }
  __syncthreads();
  packed_table_to_slab(table,slabs);
}

// One workgroup per 256 bins: thread (bin, quarter) sums a quarter of the packed slabs, the four
// partial sums meet in LDS and one thread per bin adds the total to every channel of the caller's
// table (no atomics: a bin belongs to one thread).
__global__ __launch_bounds__(1024)
void histogram_packed_reduce_kernel(const unsigned *slabs,int nblocks,unsigned long long *counts,int channels)
{
  __shared__ unsigned partial[4][256];
  const unsigned local=threadIdx.x & 255u,quarter=threadIdx.x >> 8;
  const unsigned bin=blockIdx.x*256u+local;
  const int per=(nblocks+3)/4;
  const int b0=(int) quarter*per;
  const int b1=b0+per < nblocks ? b0+per : nblocks;
  const unsigned shift=16u*(bin & 1u);
  unsigned sum=0;                              // at most 65 534 per slab: 65 536 slabs fit 32 bits
#pragma unroll 8
  for (int b=b0; b < b1; b++)
    sum+=(slabs[(size_t) b*32768+(bin >> 1)] >> shift) & 0xffffu;
  partial[quarter][local]=sum;
  __syncthreads();
  if (quarter == 0)
    {
      const unsigned long long total=(unsigned long long) partial[0][local]+partial[1][local]+partial[2][local]+partial[3][local];
      if (total != 0)
        for (int c=0; c < channels; c++)
          counts[(size_t) bin*channels+c]+=total;
    }
}

// workgroups of the packed-table kernels for a frame of n pixels (0: too many slabs)
static size_t packed_histogram_blocks(int device,size_t n)
{
  // one workgroup per CU when a share fits the 16-bit counters (plus a few pixels of slack that
  // go through global atomics), more workgroups otherwise
  size_t nblocks=(size_t) compute_units(device);
  if ((n+nblocks-1)/nblocks > kPackedCapacity+256u)
    nblocks=(n+kPackedCapacity-1)/kPackedCapacity;
  return nblocks > 65536 ? 0 : nblocks;
}

template<typename Q,int C>
static MhStatus histogram_intensity_packed(const View &src,const IntensityParams &ip,unsigned long long *hist)
{
  const size_t n=src.columns*src.rows;
  const size_t nblocks=packed_histogram_blocks(src.device,n);
  if (nblocks == 0)
    return histogram_intensity_lds<Q,C>(src,ip,hist);
  Temp slabs;
  MH_TRY(slabs.alloc(src.device,nblocks*32768*sizeof(unsigned),src.stream));
  const size_t lds=32768*sizeof(unsigned);
  const bool plain=intensity_is_plain_luma(ip,C);
  MH_HIP(hipFuncSetAttribute(plain ? reinterpret_cast<const void *>(&histogram_packed_kernel<Q,C,true>) :
    reinterpret_cast<const void *>(&histogram_packed_kernel<Q,C,false>),
    hipFuncAttributeMaxDynamicSharedMemorySize,(int) lds));
  const int wide=(C == 4) && (sizeof(Q) == 2) && ((reinterpret_cast<uintptr_t>(src.pixels) & 15u) == 0) ? 1 : 0;
  {
    ProfileScope prof("histogram",src.stream);
    if (plain)
      hipLaunchKernelGGL((histogram_packed_kernel<Q,C,true>),dim3((unsigned) nblocks),dim3(1024),lds,src.stream,
        static_cast<const Q *>(src.pixels),n,ip,slabs.as<unsigned>(),hist,wide);
    else
      hipLaunchKernelGGL((histogram_packed_kernel<Q,C,false>),dim3((unsigned) nblocks),dim3(1024),lds,src.stream,
        static_cast<const Q *>(src.pixels),n,ip,slabs.as<unsigned>(),hist,wide);
    hipLaunchKernelGGL(histogram_packed_reduce_kernel,dim3(256),dim3(1024),0,src.stream,
      slabs.as<unsigned>(),(int) nblocks,hist,C);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// sRGB -> Lab (FAST, RGBA Q16) and the intensity histogram of the Lab frame in ONE pass over the
// pixels: what TransformImageColorspace followed by ContrastStretchImage / EqualizeImage needs
// (config C4) at one frame read and one frame write.  Converts as colorspace_lab_fast_kernel
// and bins the values it stores as histogram_packed_kernel does, so the table is exactly the
// histogram of the frame it leaves behind.
__device__ __forceinline__ unsigned long long lut_block_sum(unsigned long long v,unsigned long long *shared16);
__device__ __forceinline__ double lut_scale_map_to_quantum(double value,int is_u16);

// What the levels kernels below need besides the slabs: a workgroup's pixels beyond the 16-bit
// counters' capacity as a list of bins (count first).
constexpr int kExtraPitch=264;                 // 1 + the 258 pixels a share may exceed the capacity by, padded
struct StretchScratch
{
  int black,white;                             // the levels, enhance.c:1652-1678
  unsigned apply;                              // black != white: the map is applied (enhance.c:1690)
  unsigned pad;
};

template<bool PLAIN>
__global__ __launch_bounds__(1024)
void lab_histogram_fast_kernel(uint16_t *pixels,size_t npixels,IntensityParams ip,unsigned *slabs,
  unsigned long long *counts,unsigned short *extras)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ unsigned extra_count;
  unsigned *table=reinterpret_cast<unsigned *>(smem_raw);
  float2 *decode=reinterpret_cast<float2 *>(smem_raw+32768*sizeof(unsigned));
  for (int i=(int) threadIdx.x; i < 32768; i+=1024)
    table[i]=0u;
  build_decode_table(decode);
  if (threadIdx.x == 0)
    extra_count=0u;
  __syncthreads();
  size_t per=(npixels+gridDim.x-1)/gridDim.x;
  per+=per & 1;
  size_t begin=(size_t) blockIdx.x*per;
  begin=begin < npixels ? begin : npixels;
  size_t end=begin+per;
  end=end < npixels ? end : npixels;
  const size_t packed_end=end-begin > kPackedCapacity ? begin+kPackedCapacity : end;
  auto bin_of=[&](uint2 px) -> unsigned
  {
    const uint16_t q[4]={(uint16_t) px.x,(uint16_t) (px.x >> 16),(uint16_t) px.y,(uint16_t) (px.y >> 16)};
    return QuantumOps<uint16_t>::map_index(QuantumOps<uint16_t>::clamp(pixel_intensity_of<PLAIN,uint16_t,4>(q,ip)));
  };
  auto count=[&](uint2 px)
  {
    const unsigned bin=bin_of(px);
    atomicAdd(table+(bin >> 1),(bin & 1u) != 0u ? 0x10000u : 1u);
  };
  constexpr int BATCH=8;
  uint4 *pairs=reinterpret_cast<uint4 *>(pixels)+begin/2;
  const size_t npairs=(packed_end-begin)/2;
  for (size_t i0=threadIdx.x; i0 < npairs; i0+=(size_t) 1024*BATCH)
    {
      uint4 v[BATCH];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) 1024*k;
          v[k]=pairs[i < npairs ? i : npairs-1];
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        if (i0+(size_t) 1024*k < npairs)
          {
            const uint2 first=srgb_to_lab_fast_pixel(make_uint2(v[k].x,v[k].y),decode);
            const uint2 second=srgb_to_lab_fast_pixel(make_uint2(v[k].z,v[k].w),decode);
            pairs[i0+(size_t) 1024*k]=make_uint4(first.x,first.y,second.x,second.y);
            count(first);
            count(second);
          }
    }
  // the pixels past the pairs (an odd one, or a share beyond the 16-bit counters' capacity)
  uint2 *single=reinterpret_cast<uint2 *>(pixels);
  for (size_t i=begin+2*npairs+threadIdx.x; i < end; i+=1024)
    {
      const uint2 lab=srgb_to_lab_fast_pixel(single[i],decode);
      single[i]=lab;
      if (i < packed_end)
        count(lab);
      else
        {
          const unsigned bin=bin_of(lab);
          if (extras != nullptr)
            extras[(size_t) blockIdx.x*kExtraPitch+1u+atomicAdd(&extra_count,1u)]=(unsigned short) bin;
          else
            for (int c=0; c < 4; c++)
              atomicAdd(counts+(size_t) bin*4+c,1ull);
        }
    }
  __syncthreads();
  if ((extras != nullptr) && (threadIdx.x == 0))
    extras[(size_t) blockIdx.x*kExtraPitch]=(unsigned short) extra_count;
  packed_table_to_slab(table,slabs);
}

// ContrastStretchImage's levels straight from the slabs, two small launches and no table of
// 65536 x channels 64-bit counts: stretch_bins_kernel sums the slabs (as
// histogram_packed_reduce_kernel) into 32-bit `bins` and leaves each workgroup's share (256 bins)
// in `shares`; stretch_levels_kernel, ONE workgroup, adds the listed extra pixels and finds the
// black and the white level (enhance.c:1652-1678: the first bin from below whose running count
// exceeds black_point, the last bin from above whose count exceeds white_limit) by locating the
// 1024-bin chunk from the 64 chunk sums and scanning it.  Intensity binning: all channels share
// the histogram, hence the levels.  Replaces a 2 MB memset, the slab reduction and the three LUT
// kernels; the map itself is evaluated by stretch_apply_kernel.  (One launch with a last-
// workgroup-done ticket measured 32 us: every __threadfence() writes back an L2 full of the
// frame the previous kernel stored.)
__global__ __launch_bounds__(1024)
void stretch_bins_kernel(const unsigned *slabs,int nblocks,unsigned *bins,unsigned long long *shares)
{
  // 256 bins = 32 groups of four packed words; thread (group, slice) sums every 32nd slab with
  // 16-byte loads, all in flight at once
  __shared__ unsigned partial[32][32][8];
  __shared__ unsigned long long wave_sums[16];
  {
    const int group=(int) threadIdx.x & 31,slice=(int) threadIdx.x >> 5;
    const uint4 *words=reinterpret_cast<const uint4 *>(slabs)+(size_t) blockIdx.x*32+group;
    unsigned sum[8]={0u,0u,0u,0u,0u,0u,0u,0u};     // at most 65 534 per slab: 65 536 slabs fit 32 bits
#pragma unroll 8
    for (int b=slice; b < nblocks; b+=32)
      {
        const uint4 v=words[(size_t) b*8192];
        sum[0]+=v.x & 0xffffu; sum[1]+=v.x >> 16;
        sum[2]+=v.y & 0xffffu; sum[3]+=v.y >> 16;
        sum[4]+=v.z & 0xffffu; sum[5]+=v.z >> 16;
        sum[6]+=v.w & 0xffffu; sum[7]+=v.w >> 16;
      }
#pragma unroll
    for (int k=0; k < 8; k++)
      partial[slice][group][k]=sum[k];
  }
  __syncthreads();
  unsigned long long mine=0ull;
  if (threadIdx.x < 256u)
    {
      unsigned total=0u;
#pragma unroll 8
      for (int slice=0; slice < 32; slice++)
        total+=partial[slice][threadIdx.x >> 3][threadIdx.x & 7u];
      bins[blockIdx.x*256u+threadIdx.x]=total;
      mine=total;
    }
  const unsigned long long share=lut_block_sum(mine,wave_sums);
  if (threadIdx.x == 0)
    shares[blockIdx.x]=share;
}

__global__ __launch_bounds__(1024)
void stretch_levels_kernel(const unsigned *bins,const unsigned long long *shares,const unsigned short *extras,
  int nblocks,StretchScratch *levels,double black_point,double white_limit)
{
  __shared__ unsigned long long chunk_s[64];
  __shared__ unsigned long long wave_sums[16];
  __shared__ unsigned low_s[1024],high_s[1024];    // the bins of the black and of the white chunk
  __shared__ int found_s;
  const int t=(int) threadIdx.x,lane=t & 63;
  if (t < 64)
    chunk_s[t]=shares[4*t]+shares[4*t+1]+shares[4*t+2]+shares[4*t+3];
  __syncthreads();
  // the pixels a share held beyond the packed counters' capacity (a thread per list: a couple of
  // entries each unless the shares were ragged)
  for (int w=t; w < nblocks; w+=1024)
    {
      const unsigned short *list=extras+(size_t) w*kExtraPitch;
      const int listed=(int) list[0];
      for (int i=1; i <= listed; i++)
        atomicAdd(&chunk_s[list[i] >> 10],1ull);
    }
  __syncthreads();
  // counts below each chunk (every wave computes them: 64 chunks, 64 lanes)
  const unsigned long long chunk=chunk_s[lane];
  unsigned long long inclusive=chunk;
  for (int off=1; off < 64; off<<=1)
    {
      const unsigned long long up=__shfl_up(inclusive,off,64);
      if (lane >= off)
        inclusive+=up;
    }
  const unsigned long long total=__shfl(inclusive,63,64);
  const unsigned long long below=inclusive-chunk;
  // black lies in the first chunk whose inclusive running count exceeds black_point, white in the
  // last chunk whose count from its first bin upwards exceeds white_limit
  const unsigned long long low_hit=__ballot((double) inclusive > black_point);
  const unsigned long long high_hit=__ballot((double) (total-below) > white_limit);
  const int low_chunk=low_hit != 0ull ? __builtin_ctzll(low_hit) : -1;
  const int high_chunk=high_hit != 0ull ? 63-__builtin_clzll(high_hit) : -1;
  low_s[t]=low_chunk >= 0 ? bins[low_chunk*1024+t] : 0u;
  high_s[t]=high_chunk >= 0 ? bins[high_chunk*1024+t] : 0u;
  __syncthreads();
  for (int w=t; w < nblocks; w+=1024)
    {
      const unsigned short *list=extras+(size_t) w*kExtraPitch;
      const int listed=(int) list[0];
      for (int i=1; i <= listed; i++)
        {
          const int b=(int) list[i];
          if ((b >> 10) == low_chunk)
            atomicAdd(&low_s[b & 1023],1u);
          if ((b >> 10) == high_chunk)
            atomicAdd(&high_s[b & 1023],1u);
        }
    }
  __syncthreads();
  // inclusive running count of a chunk's 1024 bins, one per thread
  auto scan=[&](unsigned long long h,unsigned long long prefix) -> unsigned long long
  {
    unsigned long long cum=h;
    for (int off=1; off < 64; off<<=1)
      {
        const unsigned long long up=__shfl_up(cum,off,64);
        if (lane >= off)
          cum+=up;
      }
    __syncthreads();
    if (lane == 63)
      wave_sums[t >> 6]=cum;
    __syncthreads();
    for (int w=0; w < (t >> 6); w++)
      cum+=wave_sums[w];
    return cum+prefix;
  };
  int black=65536;                                 // none: the reference's loop ends with j = 65536
  if (low_chunk >= 0)
    {
      const unsigned long long cum=scan(low_s[t],__shfl(below,low_chunk,64));
      if (t == 0)
        found_s=65536;
      __syncthreads();
      if ((double) cum > black_point)
        atomicMin(&found_s,low_chunk*1024+t);
      __syncthreads();
      black=found_s;
      __syncthreads();
    }
  int white=0;                                     // none
  if (high_chunk >= 0)
    {
      const unsigned long long h=high_s[t];
      const unsigned long long cum=scan(h,__shfl(below,high_chunk,64));
      if (t == 0)
        found_s=0;
      __syncthreads();
      const int j=high_chunk*1024+t;
      if ((j >= 1) && ((double) (total-(cum-h)) > white_limit))
        atomicMax(&found_s,j);
      __syncthreads();
      white=found_s;
    }
  if (t == 0)
    {
      // black[i]=(Quantum) j, enhance.c:1668: a scan that found no bin above black_point ends with
      // j = 65536, which the Q16 build stores as (unsigned short) 65536 = 0
      const int black_i=black == 65536 ? 0 : black;
      levels->black=black_i;
      levels->white=white;
      levels->apply=black_i != white ? 1u : 0u;
    }
}

// The stretch map of enhance.c:1685-1706 evaluated per sample (Q16, the levels from
// stretch_levels_kernel): no 65536-entry table to build, stage or gather from.
template<int C>
__global__ __launch_bounds__(256)
void stretch_apply_kernel(uint16_t *pixels,size_t npixels,const StretchScratch *levels,uint32_t mask)
{
  if ((levels->apply == 0u) || (mask == 0u))
    return;
  const int black_i=levels->black,white_i=levels->white;
  const double black=(double) black_i;
  const double scale=65535.0*perceptible_reciprocal((double) white_i-black);
  auto map=[&](unsigned j) -> unsigned
  {
    const double value=scale*((double) j-black);           // 65535.0*gamma*((double) j-black)
    unsigned v=(unsigned) lut_scale_map_to_quantum(value,1);
    v=(int) j > white_i ? 65535u : v;
    v=(int) j < black_i ? 0u : v;                         // (tested first in enhance.c:1694)
    return v;
  };
  constexpr int BATCH=4;
  if constexpr (C == 4)
    {
      if ((reinterpret_cast<uintptr_t>(pixels) & 15u) == 0)
        {
          // two RGBA pixels per lane and load
          uint4 *pairs=reinterpret_cast<uint4 *>(pixels);
          const size_t npairs=npixels/2;
          const size_t stride=(size_t) gridDim.x*blockDim.x*BATCH;
          for (size_t i0=(size_t) blockIdx.x*blockDim.x*BATCH+threadIdx.x; i0 < npairs; i0+=stride)
            {
              uint4 v[BATCH];
#pragma unroll
              for (int k=0; k < BATCH; k++)
                {
                  const size_t i=i0+(size_t) k*blockDim.x;
                  v[k]=pairs[i < npairs ? i : npairs-1];
                }
#pragma unroll
              for (int k=0; k < BATCH; k++)
                {
                  unsigned words[4]={v[k].x,v[k].y,v[k].z,v[k].w};
#pragma unroll
                  for (int w=0; w < 4; w++)
                    {
                      const int c0=2*(w & 1);
                      unsigned lo=words[w] & 0xffffu,hi=words[w] >> 16;
                      if ((mask >> c0) & 1u)
                        lo=map(lo);
                      if ((mask >> (c0+1)) & 1u)
                        hi=map(hi);
                      words[w]=lo | (hi << 16);
                    }
                  const size_t i=i0+(size_t) k*blockDim.x;
                  if (i < npairs)
                    pairs[i]=make_uint4(words[0],words[1],words[2],words[3]);
                }
            }
          if (((npixels & 1u) != 0) && (blockIdx.x == 0) && (threadIdx.x < 4u) && ((mask >> threadIdx.x) & 1u))
            pixels[(npixels-1)*4+threadIdx.x]=(uint16_t) map(pixels[(npixels-1)*4+threadIdx.x]);
          return;
        }
    }
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      uint16_t q[C];
      load_pixel<uint16_t,C>(pixels+i*C,q);
#pragma unroll
      for (int c=0; c < C; c++)
        if ((mask >> c) & 1u)
          q[c]=(uint16_t) map(q[c]);
      store_pixel<uint16_t,C>(pixels+i*C,q);
    }
}

// The workgroups of lab_histogram_fast_kernel for a frame that takes the fused sRGB -> Lab + packed-histogram
// route (FAST, aligned RGBA Q16, 2^20 to 2^31 pixels); 0: the frame does not qualify.
static size_t lab_histogram_fast_blocks(const View &img)
{
  const size_t n=img.columns*img.rows;
  if ((img.quantum != MH_QUANTUM_U16) || (img.channels != 4) || (precision() != MH_PRECISION_FAST) ||
      (n < ((size_t) 1 << 20)) || (n >= ((size_t) 1 << 31)) ||
      ((reinterpret_cast<uintptr_t>(img.pixels) & 15u) != 0) ||
      (option("MAGICKHIP_NO_FAST_LAB") != nullptr) || (option("MAGICKHIP_NO_PACKED_HISTOGRAM") != nullptr))
    return 0;
  return packed_histogram_blocks(img.device,n);
}

// lab_histogram_fast_kernel on nblocks workgroups.  counts != nullptr: the slabs are summed into that table
// [65536][4] as well; otherwise `extras` receives the pixels beyond the packed counters' capacity.
static MhStatus launch_lab_histogram_fast(const View &img,const MhImage *lab_desc,size_t nblocks,unsigned *slabs,
  unsigned long long *counts,unsigned short *extras)
{
  const size_t n=img.columns*img.rows;
  const IntensityParams ip=intensity_params(lab_desc);
  const size_t lds=32768*sizeof(unsigned)+kDecodePieces*sizeof(float2);
  const bool plain=intensity_is_plain_luma(ip,4);
  static bool configured[2][64]={};
  if ((img.device < 0) || (img.device >= 64) || !configured[plain ? 1 : 0][img.device])
    {
      MH_HIP(hipFuncSetAttribute(plain ? reinterpret_cast<const void *>(&lab_histogram_fast_kernel<true>) :
        reinterpret_cast<const void *>(&lab_histogram_fast_kernel<false>),
        hipFuncAttributeMaxDynamicSharedMemorySize,(int) lds));
      if ((img.device >= 0) && (img.device < 64))
        configured[plain ? 1 : 0][img.device]=true;
    }
  ProfileScope prof("colorspace_histogram",img.stream);
  if (plain)
    hipLaunchKernelGGL(lab_histogram_fast_kernel<true>,dim3((unsigned) nblocks),dim3(1024),lds,img.stream,
      static_cast<uint16_t *>(img.pixels),n,ip,slabs,counts,extras);
  else
    hipLaunchKernelGGL(lab_histogram_fast_kernel<false>,dim3((unsigned) nblocks),dim3(1024),lds,img.stream,
      static_cast<uint16_t *>(img.pixels),n,ip,slabs,counts,extras);
  if (counts != nullptr)
    hipLaunchKernelGGL(histogram_packed_reduce_kernel,dim3(256),dim3(1024),0,img.stream,
      slabs,(int) nblocks,counts,4);
  return MH_OK;
}

// *fused stays false when the frame does not qualify (the caller then runs the two operators)
MhStatus launch_lab_fast_with_histogram(const View &img,const MhImage *lab_desc,unsigned long long *hist,
  bool *fused)
{
  *fused=false;
  const size_t nblocks=lab_histogram_fast_blocks(img);
  if (nblocks == 0)
    return MH_OK;
  Temp slabs;
  MH_TRY(slabs.alloc(img.device,nblocks*32768*sizeof(unsigned),img.stream));
  MH_TRY(launch_lab_histogram_fast(img,lab_desc,nblocks,slabs.as<unsigned>(),hist,nullptr));
  MH_HIP(hipGetLastError());
  *fused=true;
  return MH_OK;
}

// FAST sRGB -> Lab followed by ContrastStretchImage on RGBA Q16 in FOUR launches: convert + bin
// (lab_histogram_fast_kernel), bins and levels (stretch_bins_kernel, stretch_levels_kernel), map
// (stretch_apply_kernel) — the general route takes seven (memset, convert + bin, slab reduction, three LUT kernels, LUT apply).
// The results are the general route's, bit for bit: the same bins, the same levels, the same map
// expression.  *fused stays false when the frame does not qualify.
MhStatus launch_lab_fast_contrast_stretch(const View &img,const MhImage *lab_desc,double black_point,
  double white_limit,uint32_t update_mask,bool *fused)
{
  *fused=false;
  const size_t n=img.columns*img.rows;
  const size_t nblocks=option("MAGICKHIP_NO_STRETCH_LEVELS") == nullptr ? lab_histogram_fast_blocks(img) : 0;
  if (nblocks == 0)
    return MH_OK;
  // one allocation: slabs, the reduced bins, the extra-pixel lists, the scratch
  const size_t slab_bytes=nblocks*32768*sizeof(unsigned);
  const size_t bins_bytes=65536*sizeof(unsigned);
  const size_t extras_bytes=((nblocks*kExtraPitch*sizeof(unsigned short))+15u) & ~(size_t) 15u;
  const size_t shares_bytes=256*sizeof(unsigned long long);
  Temp work;
  MH_TRY(work.alloc(img.device,slab_bytes+bins_bytes+extras_bytes+shares_bytes+sizeof(StretchScratch),img.stream));
  unsigned char *at=static_cast<unsigned char *>(work.ptr);
  unsigned *slabs=reinterpret_cast<unsigned *>(at);
  unsigned *bins=reinterpret_cast<unsigned *>(at+slab_bytes);
  unsigned short *extras=reinterpret_cast<unsigned short *>(at+slab_bytes+bins_bytes);
  unsigned long long *shares=reinterpret_cast<unsigned long long *>(at+slab_bytes+bins_bytes+extras_bytes);
  StretchScratch *scratch=reinterpret_cast<StretchScratch *>(at+slab_bytes+bins_bytes+extras_bytes+shares_bytes);
  MH_TRY(launch_lab_histogram_fast(img,lab_desc,nblocks,slabs,nullptr,extras));
  {
    ProfileScope prof("build_lut",img.stream);
    hipLaunchKernelGGL(stretch_bins_kernel,dim3(256),dim3(1024),0,img.stream,slabs,(int) nblocks,bins,shares);
    hipLaunchKernelGGL(stretch_levels_kernel,dim3(1),dim3(1024),0,img.stream,bins,shares,extras,(int) nblocks,
      scratch,black_point,white_limit);
  }
  {
    ProfileScope prof("apply_lut",img.stream);
    hipLaunchKernelGGL(stretch_apply_kernel<4>,dim3(stream_grid((n/2+3)/4)),dim3(256),0,img.stream,
      static_cast<uint16_t *>(img.pixels),n,scratch,update_mask);
  }
  MH_HIP(hipGetLastError());
  *fused=true;
  return MH_OK;
}

template<typename Q,int C>
static MhStatus histogram_typed(const View &src,int mode,const IntensityParams &ip,
  unsigned long long *hist)
{
  const size_t n=src.columns*src.rows;
  // large frames in intensity mode: the LDS-privatised kernel (a frame below ~1 Mpixel
  // does not amortise the 2 x 256 x 128 KB slab traffic)
  if ((mode != 0) && (n >= ((size_t) 1 << 20)))
    {
      // one pass with 16-bit counters, Q16 and float Quantum alike (the bin of a float sample is
      // ScaleQuantumToMap's)
      if ((option("MAGICKHIP_NO_PACKED_HISTOGRAM") == nullptr) && (n < ((size_t) 1 << 31)))
        return histogram_intensity_packed<Q,C>(src,ip,hist);
      return histogram_intensity_lds<Q,C>(src,ip,hist);
    }
  Temp before;
  if ((mode != 0) && (C > 1))
    {
      MH_TRY(before.alloc(src.device,65536*sizeof(unsigned long long),src.stream));
      hipLaunchKernelGGL(histogram_snapshot_kernel,dim3(256),dim3(256),0,src.stream,hist,
        before.as<unsigned long long>(),C);
    }
  {
    ProfileScope prof("histogram",src.stream);
    hipLaunchKernelGGL((histogram_kernel<Q,C>),dim3(stream_grid(n)),dim3(256),0,src.stream,
      static_cast<const Q *>(src.pixels),n,mode,ip,hist);
  }
  if ((mode != 0) && (C > 1))
    hipLaunchKernelGGL(histogram_replicate_kernel,dim3(256),dim3(256),0,src.stream,hist,
      before.as<unsigned long long>(),C);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_histogram(const View &src,int intensity_mode,const MhImage *desc,
  unsigned long long *hist)
{
  IntensityParams ip=intensity_params(desc);
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return histogram_typed<typename decltype(L)::Q,L.C>(src,intensity_mode,ip,hist); });
}

// ---------------------------------------------------------------- LUT build
// The 65536-entry scans that turn a histogram into a LUT (enhance.c:1652-1706 contrast
// stretch, :2138-2169 equalize) on the device, so the operator never waits for a histogram
// download: one workgroup per channel, 64 consecutive bins per thread, counts summed as
// 64-bit integers (the reference adds them as doubles — exact below 2^53, so the order of
// the additions does not matter) and every floating-point expression written as there.
struct LutBuildArgs
{
  const unsigned long long *hist;     // [65536][channels]
  int channels;
  int equalize;                       // 0: contrast stretch, 1: equalize
  double black_point,white_limit;     // stretch: counts; white_limit = columns*rows-white_point
  int is_u16;
  void *lut;                          // Quantum-typed [65536][channels]
  uint32_t *mask;                     // out: bit c set when channel c has black != white
  const unsigned int *colour_flag;    // optional: 0 => image is gray => leave every channel alone
  uint32_t *cdf;                      // optional (equalize): the running counts of channel cdf_column
  int cdf_column;
};

__device__ __forceinline__ double lut_scale_map_to_quantum(double value,int is_u16)
{
  // ScaleMapToQuantum, quantum-private.h:465-476, as the Quantum it is stored in
  if (value <= 0.0)
    return 0.0;
  if (value >= 65535.0)
    return 65535.0;
  if (is_u16)
    return (double) (unsigned short) (value+0.5);
  return (double) (float) value;
}

// Three small grids of (channels x 64) workgroups, one bin per thread, coalesced:
//   lut_chunk_sums_kernel   sum of each 1024-bin chunk
//   lut_scan_kernel         running count of every bin (chunk prefix + workgroup scan);
//                           equalize writes its map here, stretch records the black / white
//                           levels (first bin from below / from above whose running count
//                           passes the threshold) with one atomic per workgroup
//   lut_stretch_map_kernel  stretch map from the two levels
constexpr int kLutChunks=64;

struct LutScratch
{
  unsigned long long chunk_sum[MH_MAX_CHANNELS][kLutChunks];
  int black[MH_MAX_CHANNELS],white[MH_MAX_CHANNELS];
};

__device__ __forceinline__ bool lut_image_is_gray(const LutBuildArgs &a)
{
  return (a.colour_flag != nullptr) && (*a.colour_flag == 0);
}

__device__ __forceinline__ void lut_store(const LutBuildArgs &a,int j,int c,double v)
{
  if (a.is_u16)
    static_cast<unsigned short *>(a.lut)[(size_t) j*a.channels+c]=(unsigned short) v;
  else
    static_cast<float *>(a.lut)[(size_t) j*a.channels+c]=(float) v;
}

// workgroup-wide sum of one 64-bit value per thread (1024 threads); result in every thread
__device__ __forceinline__ unsigned long long lut_block_sum(unsigned long long v,unsigned long long *shared16)
{
  for (int off=32; off > 0; off>>=1)
    v+=__shfl_xor(v,off,64);
  if ((threadIdx.x & 63) == 0)
    shared16[threadIdx.x >> 6]=v;
  __syncthreads();
  unsigned long long total=0;
  for (int w=0; w < 16; w++)
    total+=shared16[w];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(1024)
void lut_chunk_sums_kernel(LutBuildArgs a,LutScratch *scratch)
{
  __shared__ unsigned long long wave_sums[16];
  const int c=(int) blockIdx.x,chunk=(int) blockIdx.y,j=chunk*1024+(int) threadIdx.x;
  unsigned long long total=lut_block_sum(a.hist[(size_t) j*a.channels+c],wave_sums);
  if (threadIdx.x == 0)
    {
      scratch->chunk_sum[c][chunk]=total;
      if (chunk == 0)
        {
          scratch->black[c]=65536;
          scratch->white[c]=0;
          // this channel's bit of the mask and, once, the bits above the channels (the later
          // kernels of the stream set the bit again; a memset would be one more launch)
          atomicAnd(a.mask,~(1u << c));
          if (c == 0)
            atomicAnd(a.mask,a.channels >= 32 ? 0xffffffffu : (1u << a.channels)-1u);
        }
    }
}

__global__ __launch_bounds__(1024)
void lut_scan_kernel(LutBuildArgs a,LutScratch *scratch)
{
  __shared__ unsigned long long wave_sums[16];
  __shared__ unsigned long long prefix_s,total_s;
  __shared__ int black_s,white_s;
  if (lut_image_is_gray(a))
    return;
  const int c=(int) blockIdx.x,chunk=(int) blockIdx.y,t=(int) threadIdx.x,j=chunk*1024+t;
  if (t < 64)
    {
      // wave 0: counts below this chunk, and of the whole channel
      unsigned long long v=scratch->chunk_sum[c][t];
      unsigned long long below=t < chunk ? v : 0ull;
      for (int off=32; off > 0; off>>=1)
        {
          v+=__shfl_xor(v,off,64);
          below+=__shfl_xor(below,off,64);
        }
      if (t == 0)
        {
          prefix_s=below;
          total_s=v;
          black_s=65536;
          white_s=0;
        }
    }
  const unsigned long long h=a.hist[(size_t) j*a.channels+c];
  // inclusive scan of the 1024 bins: within the wave, then across the 16 waves
  unsigned long long cum=h;
  const int lane=t & 63;
  for (int off=1; off < 64; off<<=1)
    {
      unsigned long long up=__shfl_up(cum,off,64);
      if (lane >= off)
        cum+=up;
    }
  if (lane == 63)
    wave_sums[t >> 6]=cum;
  __syncthreads();
  for (int w=0; w < (t >> 6); w++)
    cum+=wave_sums[w];
  cum+=prefix_s;
  const unsigned long long total=total_s;
  if (a.equalize != 0)
    {
      // integrate, enhance.c:2138-2152; map, :2162-2168
      const double black=(double) a.hist[c],white=(double) total;
      if ((a.cdf != nullptr) && (c == a.cdf_column))
        a.cdf[j]=(total >> 32) != 0ull ? 0xffffffffu : (uint32_t) cum;
      if (black == white)
        return;
      lut_store(a,j,c,lut_scale_map_to_quantum(
        (double) ((65535.0*((double) cum-black))/(white-black)),a.is_u16));
      if (j == 0)
        atomicOr(a.mask,1u<<c);
      return;
    }
  // black / white levels, enhance.c:1652-1678
  const unsigned long long from_top=total-(cum-h);          // bins j..65535
  if ((double) cum > a.black_point)
    atomicMin(&black_s,j);
  if ((j >= 1) && ((double) from_top > a.white_limit))
    atomicMax(&white_s,j);
  __syncthreads();
  if (t == 0)
    {
      if (black_s < 65536)
        atomicMin(&scratch->black[c],black_s);
      if (white_s > 0)
        atomicMax(&scratch->white[c],white_s);
    }
}

__global__ __launch_bounds__(1024)
void lut_stretch_map_kernel(LutBuildArgs a,const LutScratch *scratch)
{
  if (lut_image_is_gray(a))
    return;
  const int c=(int) blockIdx.x,j=(int) blockIdx.y*1024+(int) threadIdx.x;
  // black[i]=(Quantum) j, enhance.c:1668: a scan that found no bin above black_point ends with
  // j = 65536, which the Q16 build stores as (unsigned short) 65536 = 0
  const int black_i=((a.is_u16 != 0) && (scratch->black[c] == 65536)) ? 0 : scratch->black[c];
  const int white_i=scratch->white[c];
  const double black=(double) black_i,white=(double) white_i;
  // stretch map, enhance.c:1685-1706
  const double gamma=perceptible_reciprocal(white-black);
  double v=0.0;
  if (j < black_i)
    v=0.0;
  else if (j > white_i)
    v=65535.0;
  else if (black != white)
    v=lut_scale_map_to_quantum((double) (65535.0*gamma*((double) j-black)),a.is_u16);
  lut_store(a,j,c,v);
  if ((j == 0) && (black != white))
    atomicOr(a.mask,1u<<c);
}

__global__ __launch_bounds__(256)
void table_add_kernel(unsigned long long *dst,const unsigned long long *src,size_t count)
{
  for (size_t i=(size_t) blockIdx.x*256u+threadIdx.x; i < count; i+=(size_t) gridDim.x*256u)
    dst[i]+=src[i];
}

MhStatus launch_table_add(unsigned long long *dst,const unsigned long long *src,size_t count,
  int device,hipStream_t stream)
{
  DeviceGuard guard;
  MH_HIP(guard.enter(device));
  const unsigned blocks=(unsigned) ((count+255)/256 < 1024 ? (count+255)/256 : 1024);
  hipLaunchKernelGGL(table_add_kernel,dim3(blocks == 0 ? 1u : blocks),dim3(256),0,stream,dst,src,count);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_build_lut(const View &img,const unsigned long long *hist,bool equalize,
  double black_point,double white_limit,void *lut,uint32_t *mask,const unsigned int *colour_flag,
  uint32_t *cdf,int cdf_column)
{
  LutBuildArgs a;
  a.cdf=equalize ? cdf : nullptr;
  a.cdf_column=cdf_column;
  a.hist=hist;
  a.channels=img.channels;
  a.equalize=equalize ? 1 : 0;
  a.black_point=black_point;
  a.white_limit=white_limit;
  a.is_u16=img.quantum == MH_QUANTUM_U16 ? 1 : 0;
  a.lut=lut;
  a.mask=mask;
  a.colour_flag=colour_flag;
  Temp scratch;
  MH_TRY(scratch.alloc(img.device,sizeof(LutScratch),img.stream));
  const dim3 grid((unsigned) img.channels,kLutChunks);
  ProfileScope prof("build_lut",img.stream);
  hipLaunchKernelGGL(lut_chunk_sums_kernel,grid,dim3(1024),0,img.stream,a,scratch.as<LutScratch>());
  hipLaunchKernelGGL(lut_scan_kernel,grid,dim3(1024),0,img.stream,a,scratch.as<LutScratch>());
  if (!equalize)
    hipLaunchKernelGGL(lut_stretch_map_kernel,grid,dim3(1024),0,img.stream,a,scratch.as<LutScratch>());
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ContrastStretchImage without the 65536 x channels table: the two scan kernels above leave the
// black and the white level of every channel in the scratch block, and this kernel evaluates
// enhance.c:1685-1706's map per sample (as lut_stretch_map_kernel would have tabulated it — the
// same expressions, so the same bits) for Q16 and float Quantum, any channel count, intensity or
// per-channel binning.  A float frame gathered four floats per pixel from a 1 MB table before
// (1.4 ms per 8192^2 RGBA frame); a Q16 frame staged a 128 KB column in LDS per workgroup.
template<typename Q,int C>
__global__ __launch_bounds__(256)
void stretch_apply_levels_kernel(Q *pixels,size_t npixels,const LutScratch *scratch,uint32_t mask,
  const unsigned int *colour_flag)
{
  if ((colour_flag != nullptr) && (*colour_flag == 0))
    return;                                      // the image is gray: every channel is left alone
  constexpr int is_u16=sizeof(Q) == 2 ? 1 : 0;
  int black_i[C],white_i[C];
  double black[C],scale[C];
  uint32_t apply=0;
#pragma unroll
  for (int c=0; c < C; c++)
    {
      // black[i]=(Quantum) j, enhance.c:1668: a scan that found no bin above black_point ends with
      // j = 65536, which the Q16 build stores as (unsigned short) 65536 = 0
      black_i[c]=((is_u16 != 0) && (scratch->black[c] == 65536)) ? 0 : scratch->black[c];
      white_i[c]=scratch->white[c];
      black[c]=(double) black_i[c];
      scale[c]=65535.0*perceptible_reciprocal((double) white_i[c]-black[c]);
      if ((black_i[c] != white_i[c]) && (((mask >> c) & 1u) != 0u))
        apply|=1u << c;
    }
  if (apply == 0u)
    return;
  constexpr int BATCH=4;
  const size_t stride=(size_t) gridDim.x*blockDim.x*BATCH;
  for (size_t i0=(size_t) blockIdx.x*blockDim.x*BATCH+threadIdx.x; i0 < npixels; i0+=stride)
    {
      Q q[BATCH][C];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) k*blockDim.x;
          load_pixel<Q,C>(pixels+(i < npixels ? i : npixels-1)*C,q[k]);
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) k*blockDim.x;
          if (i >= npixels)
            continue;
#pragma unroll
          for (int c=0; c < C; c++)
            if ((apply >> c) & 1u)
              {
                const int j=(int) QuantumOps<Q>::map_index(q[k][c]);
                double v=lut_scale_map_to_quantum(scale[c]*((double) j-black[c]),is_u16);   // 65535.0*gamma*((double) j-black)
                v=j > white_i[c] ? 65535.0 : v;
                v=j < black_i[c] ? 0.0 : v;        // (tested first in enhance.c:1694)
                q[k][c]=(Q) v;
              }
          store_pixel<Q,C>(pixels+i*C,q[k]);
        }
    }
}

// levels of every channel from the table [65536][channels], then the map: three launches
MhStatus launch_stretch_levels_apply(const View &img,const unsigned long long *hist,double black_point,
  double white_limit,uint32_t update_mask,const unsigned int *colour_flag)
{
  LutBuildArgs a;
  a.hist=hist;
  a.channels=img.channels;
  a.equalize=0;
  a.cdf=nullptr;
  a.cdf_column=0;
  a.black_point=black_point;
  a.white_limit=white_limit;
  a.is_u16=img.quantum == MH_QUANTUM_U16 ? 1 : 0;
  a.lut=nullptr;
  a.colour_flag=colour_flag;
  Temp scratch;
  MH_TRY(scratch.alloc(img.device,sizeof(LutScratch)+sizeof(uint32_t),img.stream));
  LutScratch *levels=scratch.as<LutScratch>();
  a.mask=reinterpret_cast<uint32_t *>(levels+1);   // (the scan kernels keep their mask word)
  const dim3 grid((unsigned) img.channels,kLutChunks);
  {
    ProfileScope prof("build_lut",img.stream);
    hipLaunchKernelGGL(lut_chunk_sums_kernel,grid,dim3(1024),0,img.stream,a,levels);
    hipLaunchKernelGGL(lut_scan_kernel,grid,dim3(1024),0,img.stream,a,levels);
  }
  const size_t n=img.columns*img.rows;
  {
    ProfileScope prof("apply_lut",img.stream);
    const dim3 apply_grid(stream_grid((n+3)/4)),block(256);
    dispatch_layout(img.quantum,img.channels,[&](auto L) {
      using Q=typename decltype(L)::Q;
      hipLaunchKernelGGL((stretch_apply_levels_kernel<Q,L.C>),apply_grid,block,0,img.stream,
        static_cast<Q *>(img.pixels),n,levels,update_mask,colour_flag); });
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ---------------------------------------------------------------- LUT apply
template<typename Q,int C>
__global__ __launch_bounds__(256)
void apply_lut_kernel(Q *pixels,size_t npixels,const Q *lut,uint32_t mask,
  const uint32_t *device_mask,int lut_stride,int column_step)
{
  if (device_mask != nullptr)
    mask&=*device_mask;                 // uniform: written by build_lut_kernel earlier in the stream
  if (mask == 0)
    return;
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
#pragma unroll
      for (int c=0; c < C; c++)
        if ((mask >> c) & 1u)
          q[c]=lut[(size_t) QuantumOps<Q>::map_index(q[c])*lut_stride+c*column_step];
      store_pixel<Q,C>(pixels+i*C,q);
    }
}

template<typename Q,int C>
static MhStatus apply_lut_typed(const View &img,const void *lut,uint32_t mask,
  const uint32_t *device_mask,bool single_column=false,const char *label="apply_lut")
{
  const size_t n=img.columns*img.rows;
  ProfileScope prof(label,img.stream);
  hipLaunchKernelGGL((apply_lut_kernel<Q,C>),dim3(stream_grid(n)),dim3(256),0,img.stream,
    static_cast<Q *>(img.pixels),n,static_cast<const Q *>(lut),mask,device_mask,
    single_column ? 1 : C,single_column ? 0 : 1);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// Q16, every masked channel maps through the SAME 65536-entry column (the intensity-
// binned operators give all channels one histogram, hence one LUT: enhance.c:1637-1643):
// the 128 KB column lives in LDS of a persistent workgroup per CU and the 4 lookups per
// pixel are LDS reads instead of scattered 2-byte global gathers.
template<int C>
__global__ __launch_bounds__(1024)
void apply_lut_shared_kernel(uint16_t *pixels,size_t npixels,const uint16_t *lut,int column,uint32_t mask,
  const uint32_t *device_mask,int lut_stride)
{
  if (device_mask != nullptr)
    mask&=*device_mask;
  if (mask == 0)
    return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint16_t *table=reinterpret_cast<uint16_t *>(smem_raw);
  for (int i=(int) threadIdx.x; i < 65536; i+=1024)
    table[i]=lut[(size_t) i*lut_stride+column];
  __syncthreads();
  constexpr int BATCH=4;
  const size_t stride=(size_t) gridDim.x*1024*BATCH;
  for (size_t i0=(size_t) blockIdx.x*1024*BATCH+threadIdx.x; i0 < npixels; i0+=stride)
    {
      uint16_t q[BATCH][C];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          size_t i=i0+(size_t) 1024*k;
          load_pixel<uint16_t,C>(pixels+(i < npixels ? i : npixels-1)*C,q[k]);
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          size_t i=i0+(size_t) 1024*k;
          if (i < npixels)
            {
#pragma unroll
              for (int c=0; c < C; c++)
                if ((mask >> c) & 1u)
                  q[k][c]=table[q[k][c]];
              store_pixel<uint16_t,C>(pixels+i*C,q[k]);
            }
        }
    }
}

template<int C>
static MhStatus apply_lut_shared(const View &img,const void *lut,int column,uint32_t mask,
  const uint32_t *device_mask,bool single_column=false,const char *label="apply_lut")
{
  const size_t n=img.columns*img.rows;
  const int cus=compute_units(img.device);
  const size_t lds=65536*sizeof(uint16_t);
  MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&apply_lut_shared_kernel<C>),
    hipFuncAttributeMaxDynamicSharedMemorySize,(int) lds));
  ProfileScope prof(label,img.stream);
  hipLaunchKernelGGL((apply_lut_shared_kernel<C>),dim3(cus),dim3(1024),lds,img.stream,
    static_cast<uint16_t *>(img.pixels),n,static_cast<const uint16_t *>(lut),single_column ? 0 : column,mask,
    device_mask,single_column ? 1 : C);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// EqualizeImage on a float frame whose channels share one histogram (intensity binning: the
// default, synchronised channels).  Its map is  ScaleMapToQuantum(65535*(cum[j]-black)/(white-black))
// (enhance.c:2162-2168) with INTEGER running counts cum[j]: 65536 floats of table (256 KB, a
// gather through L2 per sample: 0.32 ms per 4096^2 RGBA frame) do not fit the LDS, the counts do —
// a uint32 every 16 bins (16 KB) and a uint16 offset per bin (128 KB) — and the map is three
// fp64 operations on them, the table's own, so the same bits.  A 16-bin group that holds more than
// 65535 pixels (a frame with a flat background) or a frame of 2^32 pixels sends the workgroup to
// the tabulated map.
template<int C>
__global__ __launch_bounds__(1024)
void equalize_cdf_apply_kernel(float *pixels,size_t npixels,const uint32_t *cdf,const float *lut,int column,
  uint32_t mask,const uint32_t *device_mask)
{
  if (device_mask != nullptr)
    mask&=*device_mask;                 // (zero: gray frame, or black == white)
  if (mask == 0)
    return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint32_t *base=reinterpret_cast<uint32_t *>(smem_raw);                     // [4096]
  uint16_t *offset=reinterpret_cast<uint16_t *>(smem_raw+4096*sizeof(uint32_t));   // [65536]
  __shared__ int overflow;
  if (threadIdx.x == 0)
    overflow=cdf[65535] == 0xffffffffu ? 1 : 0;
  __syncthreads();
  for (int j=(int) threadIdx.x; j < 65536; j+=1024)
    {
      const uint32_t count=cdf[j],first=cdf[j & ~15];
      const uint32_t d=count-first;
      if (d > 65535u)
        overflow=1;                     // (every writer writes the same 1)
      offset[j]=(uint16_t) d;
      if ((j & 15) == 0)
        base[j >> 4]=count;
    }
  __syncthreads();
  const bool tabulated=overflow != 0;
  const double black=(double) cdf[0],white=(double) cdf[65535];
  constexpr int BATCH=4;
  const size_t stride=(size_t) gridDim.x*1024*BATCH;
  for (size_t i0=(size_t) blockIdx.x*1024*BATCH+threadIdx.x; i0 < npixels; i0+=stride)
    {
      float q[BATCH][C];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) 1024*k;
          load_pixel<float,C>(pixels+(i < npixels ? i : npixels-1)*C,q[k]);
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) 1024*k;
          if (i < npixels)
            {
#pragma unroll
              for (int c=0; c < C; c++)
                if ((mask >> c) & 1u)
                  {
                    const unsigned j=QuantumOps<float>::map_index(q[k][c]);
                    if (tabulated)
                      {
                        q[k][c]=lut[(size_t) j*C+column];
                        continue;
                      }
                    const double cum=(double) (base[j >> 4]+(uint32_t) offset[j]);
                    const double value=(65535.0*(cum-black))/(white-black);
                    q[k][c]=value <= 0.0 ? 0.0f : (value >= 65535.0 ? 65535.0f : (float) value);
                  }
              store_pixel<float,C>(pixels+i*C,q[k]);
            }
        }
    }
}

MhStatus launch_equalize_cdf_apply(const View &img,const uint32_t *cdf,const void *lut,uint32_t apply_mask,
  const Roles &roles,int shared_column,const uint32_t *device_mask)
{
  if ((img.channels < 1) || (img.channels > 4))
    return fail(MH_UNSUPPORTED,"%d channels",img.channels);
  const uint32_t mask=apply_mask & roles.update_mask;
  const size_t n=img.columns*img.rows;
  const int cus=compute_units(img.device);
  const size_t lds=4096*sizeof(uint32_t)+65536*sizeof(uint16_t);
  float *pixels=static_cast<float *>(img.pixels);
  const float *table=static_cast<const float *>(lut);
  return dispatch_channels(img.channels,[&](auto c) -> MhStatus {
    MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&equalize_cdf_apply_kernel<c.value>),
      hipFuncAttributeMaxDynamicSharedMemorySize,(int) lds));
    {
      ProfileScope prof("apply_lut",img.stream);
      hipLaunchKernelGGL((equalize_cdf_apply_kernel<c.value>),dim3(cus),dim3(1024),lds,img.stream,pixels,n,cdf,table,
        shared_column,mask,device_mask);
    }
    MH_HIP(hipGetLastError());
    return MH_OK; });
}

MhStatus launch_apply_lut(const View &img,const void *lut,uint32_t apply_mask,const Roles &roles,
  int shared_column,const uint32_t *device_mask,bool single_column,const char *label)
{
  uint32_t mask=apply_mask & roles.update_mask;
  if (single_column)
    shared_column=0;
  if ((shared_column >= 0) && (img.quantum == MH_QUANTUM_U16) &&
      (img.columns*img.rows >= ((size_t) 1 << 20)))
    return dispatch_channels(img.channels,[&](auto c) {
      return apply_lut_shared<c.value>(img,lut,shared_column,mask,device_mask,single_column,label); });
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    return apply_lut_typed<typename decltype(L)::Q,L.C>(img,lut,mask,device_mask,single_column,label); });
}

} // namespace mh
