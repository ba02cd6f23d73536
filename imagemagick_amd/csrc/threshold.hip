// The threshold operators of MagickCore/threshold.c, bit-identical to the reference on Q16 and float
// Quantum in both precision modes (every result is a comparison: there is no FAST variant).
//
//   BilevelImage :805-896, BlackThresholdImage :927-1058, WhiteThresholdImage :2518-2648,
//   RangeThresholdImage :2377-2487: `pixel` = GetPixelIntensity, formed once per pixel, replaced by
//   the channel's own sample when channel_mask != AllChannels; only channels with the Update trait
//   are written.
//   AutoThresholdImage :660-762: 256 counts of ScaleQuantumToChar(ClampToQuantum(intensity)); the
//   selection runs on the host (operators_enhance.cpp), then BilevelImage.
//   AdaptiveThresholdImage :182-361: output (x,y) = centre <= sum/(W*H)+bias ? 0 : QuantumRange over
//   the W x H window with top-left corner (x-W/2, y-H/2), edge-clamped; Copy channels take the centre.
//
// MI355X mapping:
//   threshold_point_kernel      one lane per pixel, one vector load and one vector store
//   threshold_histogram_kernel  256 LDS counters per workgroup; lanes of a wave that agree on the bin
//                               fold into one LDS atomic; non-zero counters merge into 256 uint64
//                               words with vector atomics
//   adaptive_q16_kernel         exact integer window sums.  A workgroup of kAdaptiveThreads lanes owns
//                               a strip of kAdaptiveSpan input columns (kAdaptiveLaneColumns per lane),
//                               that is kAdaptiveSpan-(W-1) output columns, and walks down a band of
//                               rows.  Every lane keeps the vertical H-sum of its columns in registers
//                               (+= entering row, -= leaving row; uint32: H*65535 < 2^32); per row the
//                               strip's inclusive prefix sum goes to LDS (uint64, two barriers a row) and an output is one
//                               subtraction, one fp64 division, one add, one compare.  Every term is an
//                               integer below 2^16 and W*H*65535 < 2^53, so the reference's running fp64
//                               sum is this integer in any order.
//                               Limits (MH_UNSUPPORTED): W > kAdaptiveMaxWidth = kAdaptiveSpan/2+1 = 257,
//                               H > kAdaptiveMaxHeight = 65537.  No LDS limit on H.  A band is
//                               max(kAdaptiveBandRows, 4*H) rows and costs H-1 warm-up rows.
//   adaptive_float_kernel       the reference's chain statement for statement: one lane carries one
//                               (row, channel) from column 0 to the end of the row, since the running
//                               sum carries its rounding along the row.  Loads rely on the caches.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "pixel_intensity.hpp"

#include <algorithm>

namespace mh {

constexpr int kThresholdThreads=256;
constexpr unsigned kThresholdMaxBlocks=1u << 20;

enum { TH_BILEVEL=0,TH_BLACK=1,TH_WHITE=2,TH_RANGE=3 };

struct ThresholdArgs
{
  void *pixels;
  unsigned long long count;            // pixels
  int mode;                            // TH_*
  int per_channel;                     // channel_mask != AllChannels: the channel's own sample decides
  uint32_t update_mask;
  double thresholds[MH_MAX_CHANNELS];  // TH_BILEVEL: [0]; TH_BLACK / TH_WHITE: per stored channel
  double low_black,low_white,high_white,high_black;
  double low_scale,high_scale;         // QuantumRange*PerceptibleReciprocal(low_white-low_black), ... (high_black-high_white)
  IntensityParams ip;
};

template<typename Q>
static __device__ __forceinline__ Q threshold_sample(const ThresholdArgs &a,int c,double pixel,Q q)
{
  switch (a.mode)
  {
    case TH_BILEVEL:
      return (Q) (pixel <= a.thresholds[0] ? 0 : 65535);
    case TH_BLACK:
      return pixel < a.thresholds[c] ? (Q) 0 : q;
    case TH_WHITE:
      return pixel > a.thresholds[c] ? (Q) 65535 : q;
    default:
      break;
  }
  // threshold.c:2446-2464, branch for branch
  if (pixel < a.low_black)
    return (Q) 0;
  if ((pixel >= a.low_black) && (pixel < a.low_white))
    return QuantumOps<Q>::clamp(a.low_scale*(pixel-a.low_black));
  if ((pixel >= a.low_white) && (pixel <= a.high_white))
    return (Q) 65535;
  if ((pixel > a.high_white) && (pixel <= a.high_black))
    return QuantumOps<Q>::clamp(a.high_scale*(a.high_black-pixel));
  return (Q) 0;
}

template<typename Q,int C>
__global__ __launch_bounds__(kThresholdThreads)
void threshold_point_kernel(ThresholdArgs a)
{
  Q *pixels=static_cast<Q *>(a.pixels);
  const unsigned long long stride=(unsigned long long) gridDim.x*kThresholdThreads;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kThresholdThreads+threadIdx.x; i < a.count; i+=stride)
    {
      Q q[C],out[C];
      load_pixel<Q,C>(pixels+i*C,q);
      const double intensity=a.per_channel ? 0.0 : pixel_intensity<Q,C>(q,a.ip);
#pragma unroll
      for (int c=0; c < C; c++)
        {
          out[c]=q[c];
          if (((a.update_mask >> c) & 1u) != 0)
            out[c]=threshold_sample<Q>(a,c,a.per_channel ? (double) q[c] : intensity,q[c]);
        }
      store_pixel<Q,C>(pixels+i*C,out);
    }
}

// ScaleQuantumToChar(ClampToQuantum(intensity)), quantum.h:86-97 and :113-124
template<typename Q>
static __device__ __forceinline__ unsigned threshold_bin(double intensity)
{
  if constexpr (QuantumOps<Q>::is_float)
    {
      const float q=(float) intensity;
      if (!(q > 0.0f))
        return 0u;
      // q/257.0f: the quotient of two floats formed in fp64 and rounded once more is the correctly
      // rounded float quotient (53 >= 2*24+2)
      const float scaled=(float) ((double) q/257.0);
      if (scaled >= 255.0f)
        return 255u;
      return (unsigned) __fadd_rn(scaled,0.5f) & 0xffu;
    }
  else
    {
      const unsigned q=QuantumOps<uint16_t>::clamp(intensity);
      return (((q+128u)-((q+128u) >> 8)) >> 8) & 0xffu;
    }
}

// one count into an LDS histogram; every lane of the wave calls this together.  Lanes that agree on
// the bin fold into one atomic (a constant frame: one per wave instead of 64 on one address).
static __device__ __forceinline__ void threshold_count(uint32_t *histogram,unsigned bin,bool valid)
{
  const int lane=(int) (threadIdx.x & 63);
  const unsigned neighbour=__shfl(bin,(lane+1) & 63,64);
  const unsigned long long agree=__ballot(valid && (neighbour == bin));
  if (__popcll(agree) < 16)
    {
      if (valid)
        atomicAdd(histogram+bin,1u);
      return;
    }
  unsigned long long remaining=__ballot(valid);
  while (remaining != 0)
    {
      const int leader=__ffsll((long long) remaining)-1;
      const unsigned leader_bin=__shfl(bin,leader,64);
      const unsigned long long same=__ballot(valid && (bin == leader_bin)) & remaining;
      if (lane == leader)
        atomicAdd(histogram+leader_bin,(uint32_t) __popcll(same));
      remaining&=~same;
    }
}

struct ThresholdHistogramArgs
{
  const void *pixels;
  unsigned long long count;
  unsigned long long *counts;          // [256], zeroed
  IntensityParams ip;
};

template<typename Q,int C>
__global__ __launch_bounds__(kThresholdThreads)
void threshold_histogram_kernel(ThresholdHistogramArgs a)
{
  __shared__ uint32_t histogram[256];
  histogram[threadIdx.x]=0u;
  __syncthreads();
  const Q *pixels=static_cast<const Q *>(a.pixels);
  const unsigned long long stride=(unsigned long long) gridDim.x*kThresholdThreads;
  // whole rounds: every lane of a wave reaches threshold_count together
  const unsigned long long first=(unsigned long long) blockIdx.x*kThresholdThreads;
  for (unsigned long long base=first; base < a.count; base+=stride)
    {
      const unsigned long long i=base+threadIdx.x;
      const bool valid=i < a.count;
      unsigned bin=0u;
      if (valid)
        {
          Q q[C];
          load_pixel<Q,C>(pixels+i*C,q);
          bin=threshold_bin<Q>(pixel_intensity<Q,C>(q,a.ip));
        }
      threshold_count(histogram,bin,valid);
    }
  __syncthreads();
  const uint32_t count=histogram[threadIdx.x];
  if (count != 0u)
    atomicAdd(a.counts+threadIdx.x,(unsigned long long) count);
}

// ------------------------------------------------------------------ AdaptiveThresholdImage
constexpr int kAdaptiveThreads=256;
constexpr int kAdaptiveLaneColumns=2;
constexpr int kAdaptiveSpan=kAdaptiveThreads*kAdaptiveLaneColumns;   // input columns of a strip
constexpr int kAdaptiveMaxWidth=kAdaptiveSpan/2+1;                   // 257: a strip keeps 256 outputs
constexpr int kAdaptiveMaxHeight=65537;                              // H*65535 < 2^32
constexpr int kAdaptiveBandRows=64;                                  // a band: max(this, 4*H) rows
constexpr int kAdaptiveWaves=kAdaptiveThreads/64;
constexpr int kAdaptiveFloatThreads=64;
constexpr long long kAdaptiveFloatMaxSide=1 << 20;                   // float Quantum: int coordinates

struct AdaptiveArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int width,height;          // W, H >= 1
  int outputs;               // output columns of a strip: kAdaptiveSpan-(W-1)
  int band;                  // rows of a band
  uint32_t copy_mask;
  double number_pixels;      // (double) (W*H)
  double bias;
};

template<typename Q,int C>
__global__ __launch_bounds__(kAdaptiveThreads)
void adaptive_q16_kernel(AdaptiveArgs a)
{
  // one buffer each: a row's two barriers also order the next row's writes behind this row's reads
  __shared__ unsigned long long prefix[C][kAdaptiveSpan];
  __shared__ unsigned long long totals[C][kAdaptiveWaves];
  const Q *src=static_cast<const Q *>(a.src);
  Q *dst=static_cast<Q *>(a.dst);
  const int t=(int) threadIdx.x,lane=t & 63,wave=t >> 6;
  const int x0=(int) blockIdx.x*a.outputs;                 // first output column of the strip
  const int y0=(int) blockIdx.y*a.band;
  const int y1=min(y0+a.band,a.rows);
  const int left=x0-a.width/2;                             // frame column of the strip's input column 0
  // this lane's input columns, edge-clamped
  size_t column[kAdaptiveLaneColumns];
#pragma unroll
  for (int k=0; k < kAdaptiveLaneColumns; k++)
    column[k]=(size_t) min(max(left+kAdaptiveLaneColumns*t+k,0),a.columns-1)*C;
  const size_t pitch=(size_t) a.columns*C;
  // the vertical sums of the window of row y0, less its last row
  uint32_t sums[kAdaptiveLaneColumns][C];
#pragma unroll
  for (int k=0; k < kAdaptiveLaneColumns; k++)
#pragma unroll
    for (int c=0; c < C; c++)
      sums[k][c]=0u;
  const int top=y0-a.height/2;
  for (int v=0; v < a.height-1; v++)
    {
      const Q *row=src+(size_t) min(max(top+v,0),a.rows-1)*pitch;
#pragma unroll
      for (int k=0; k < kAdaptiveLaneColumns; k++)
        {
          Q q[C];
          load_pixel<Q,C>(row+column[k],q);
#pragma unroll
          for (int c=0; c < C; c++)
            sums[k][c]+=(uint32_t) q[c];
        }
    }
  for (int y=y0; y < y1; y++)
    {
      // the window's last row enters
      {
        const Q *row=src+(size_t) min(max(y-a.height/2+a.height-1,0),a.rows-1)*pitch;
#pragma unroll
        for (int k=0; k < kAdaptiveLaneColumns; k++)
          {
            Q q[C];
            load_pixel<Q,C>(row+column[k],q);
#pragma unroll
            for (int c=0; c < C; c++)
              sums[k][c]+=(uint32_t) q[c];
          }
      }
      // inclusive prefix sum over the strip's kAdaptiveSpan columns: lane, wave, workgroup
      unsigned long long scan[C];
#pragma unroll
      for (int c=0; c < C; c++)
        {
          unsigned long long s=0;
#pragma unroll
          for (int k=0; k < kAdaptiveLaneColumns; k++)
            s+=(unsigned long long) sums[k][c];
#pragma unroll
          for (int off=1; off < 64; off<<=1)
            {
              const unsigned long long other=__shfl_up(s,off,64);
              if (lane >= off)
                s+=other;
            }
          scan[c]=s;
          if (lane == 63)
            totals[c][wave]=s;
        }
      __syncthreads();
#pragma unroll
      for (int c=0; c < C; c++)
        {
          unsigned long long s=scan[c];
          for (int w=0; w < wave; w++)
            s+=totals[c][w];
          // s: inclusive through this lane's last column
#pragma unroll
          for (int k=kAdaptiveLaneColumns-1; k >= 0; k--)
            {
              prefix[c][kAdaptiveLaneColumns*t+k]=s;
              s-=(unsigned long long) sums[k][c];
            }
        }
      __syncthreads();
      // outputs: strip column o is the window of input columns o ... o+W-1
      {
        const Q *centre_row=src+(size_t) y*pitch;
        Q *out_row=dst+(size_t) y*pitch;
        for (int o=t; o < a.outputs; o+=kAdaptiveThreads)
          {
            const int x=x0+o;
            if (x >= a.columns)
              break;
            Q q[C],out[C];
            load_pixel<Q,C>(centre_row+(size_t) x*C,q);
#pragma unroll
            for (int c=0; c < C; c++)
              {
                out[c]=q[c];
                if (((a.copy_mask >> c) & 1u) == 0)
                  {
                    const unsigned long long sum=prefix[c][o+a.width-1]-(o > 0 ? prefix[c][o-1] : 0ull);
                    const double mean=(double) sum/a.number_pixels+a.bias;
                    out[c]=(Q) ((double) q[c] <= mean ? 0 : 65535);
                  }
              }
            store_pixel<Q,C>(out_row+(size_t) x*C,out);
          }
      }
      // the window's first row leaves
      {
        const Q *row=src+(size_t) min(max(y-a.height/2,0),a.rows-1)*pitch;
#pragma unroll
        for (int k=0; k < kAdaptiveLaneColumns; k++)
          {
            Q q[C];
            load_pixel<Q,C>(row+column[k],q);
#pragma unroll
            for (int c=0; c < C; c++)
              sums[k][c]-=(uint32_t) q[c];
          }
      }
    }
}

// threshold.c:273-334 for one (row, channel), statement for statement
template<typename Q,int C>
__global__ __launch_bounds__(kAdaptiveFloatThreads)
void adaptive_float_kernel(AdaptiveArgs a)
{
  const Q *src=static_cast<const Q *>(a.src);
  Q *dst=static_cast<Q *>(a.dst);
  const unsigned long long chain=(unsigned long long) blockIdx.x*kAdaptiveFloatThreads+threadIdx.x;
  if (chain >= (unsigned long long) a.rows*C)
    return;
  const int y=(int) (chain/C),c=(int) (chain-(unsigned long long) y*C);
  const size_t pitch=(size_t) a.columns*C;
  const Q *centre=src+(size_t) y*pitch+c;
  Q *out=dst+(size_t) y*pitch+c;
  if (((a.copy_mask >> c) & 1u) != 0)
    {
      for (int x=0; x < a.columns; x++)
        out[(size_t) x*C]=centre[(size_t) x*C];
      return;
    }
  const int W=a.width,H=a.height;
  const int top=y-H/2,last=a.columns-1,bottom=a.rows-1;
  double channel_bias=0.0,channel_sum=0.0;
  for (int v=0; v < H; v++)
    {
      const Q *row=src+(size_t) min(max(top+v,0),bottom)*pitch+c;
      for (int u=0; u < W; u++)
        {
          const double sample=(double) row[(size_t) min(max(u-W/2,0),last)*C];
          if (u == W-1)
            channel_bias+=sample;
          channel_sum+=sample;
        }
    }
  for (int x=0; x < a.columns; x++)
    {
      channel_sum-=channel_bias;
      channel_bias=0.0;
      const size_t first_column=(size_t) min(max(x-W/2,0),last)*C;
      const size_t last_column=(size_t) min(max(x-W/2+W-1,0),last)*C;
      for (int v=0; v < H; v++)
        {
          const Q *row=src+(size_t) min(max(top+v,0),bottom)*pitch+c;
          channel_bias+=(double) row[first_column];
          channel_sum+=(double) row[last_column];
        }
      const double mean=channel_sum/a.number_pixels+a.bias;
      out[(size_t) x*C]=(Q) ((double) centre[(size_t) x*C] <= mean ? 0 : 65535);
    }
}

// ------------------------------------------------------------------ launchers
static MhStatus threshold_point(const View &img,ThresholdArgs &a,const MhImage *desc,const char *name)
{
  if ((img.columns == 0) || (img.rows == 0))
    return MH_OK;
  a.pixels=img.pixels;
  a.count=(unsigned long long) img.columns*(unsigned long long) img.rows;
  a.per_channel=desc->channel_mask != MH_ALL_CHANNELS ? 1 : 0;
  a.update_mask=0;
  for (uint32_t c=0; c < desc->number_channels; c++)
    if ((desc->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
      a.update_mask|=1u << c;
  a.ip=intensity_params(desc);
  const unsigned blocks=(unsigned) std::min<unsigned long long>((a.count+kThresholdThreads-1)/kThresholdThreads,
    kThresholdMaxBlocks);
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    ProfileScope prof(name,img.stream);
    hipLaunchKernelGGL((threshold_point_kernel<typename decltype(L)::Q,L.C>),dim3(blocks),dim3(kThresholdThreads),0,
      img.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

MhStatus launch_bilevel(const View &img,double threshold,const MhImage *desc)
{
  ThresholdArgs a={};
  a.mode=TH_BILEVEL;
  a.thresholds[0]=threshold;
  return threshold_point(img,a,desc,"threshold_bilevel");
}

MhStatus launch_black_white_threshold(const View &img,bool white,const double *thresholds,const MhImage *desc)
{
  ThresholdArgs a={};
  a.mode=white ? TH_WHITE : TH_BLACK;
  for (int c=0; c < MH_MAX_CHANNELS; c++)
    a.thresholds[c]=thresholds[c];
  return threshold_point(img,a,desc,white ? "threshold_white" : "threshold_black");
}

MhStatus launch_range_threshold(const View &img,double low_black,double low_white,double high_white,
  double high_black,double low_scale,double high_scale,const MhImage *desc)
{
  ThresholdArgs a={};
  a.mode=TH_RANGE;
  a.low_black=low_black;
  a.low_white=low_white;
  a.high_white=high_white;
  a.high_black=high_black;
  a.low_scale=low_scale;
  a.high_scale=high_scale;
  return threshold_point(img,a,desc,"threshold_range");
}

MhStatus launch_threshold_histogram(const View &img,const MhImage *desc,unsigned long long *counts_device)
{
  MH_HIP(hipMemsetAsync(counts_device,0,256*sizeof(unsigned long long),img.stream));
  if ((img.columns == 0) || (img.rows == 0))
    return MH_OK;
  ThresholdHistogramArgs a={};
  a.pixels=img.pixels;
  a.count=(unsigned long long) img.columns*(unsigned long long) img.rows;
  a.counts=counts_device;
  a.ip=intensity_params(desc);
  // 16 rounds of a workgroup at the least, and at most eight workgroups a compute unit: the merge is
  // 256 atomics a workgroup
  const unsigned long long wanted=(a.count+16ull*kThresholdThreads-1)/(16ull*kThresholdThreads);
  const unsigned blocks=(unsigned) std::max<unsigned long long>(1,
    std::min<unsigned long long>(wanted,8ull*(unsigned long long) compute_units(img.device)));
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    ProfileScope prof("threshold_histogram",img.stream);
    hipLaunchKernelGGL((threshold_histogram_kernel<typename decltype(L)::Q,L.C>),dim3(blocks),dim3(kThresholdThreads),0,
      img.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

static MhStatus adaptive_plan(const View &src,size_t width,size_t height,AdaptiveArgs *a,dim3 *grid)
{
  if ((src.columns > 0x3fffffffu) || (src.rows > 0x3fffffffu))
    return fail(MH_UNSUPPORTED,"AdaptiveThresholdImage: %zux%zu frame",src.columns,src.rows);
  a->columns=(int) src.columns;
  a->rows=(int) src.rows;
  if (src.quantum == MH_QUANTUM_U16)
    {
      if ((width > (size_t) kAdaptiveMaxWidth) || (height > (size_t) kAdaptiveMaxHeight))
        return fail(MH_UNSUPPORTED,"AdaptiveThresholdImage: a %zux%zu window (Q16: at most %dx%d)",width,height,
          kAdaptiveMaxWidth,kAdaptiveMaxHeight);
      a->outputs=kAdaptiveSpan-((int) width-1);
      a->band=std::max(kAdaptiveBandRows,4*(int) height);
      const size_t strips=(src.columns+(size_t) a->outputs-1)/(size_t) a->outputs;
      const size_t bands=(src.rows+(size_t) a->band-1)/(size_t) a->band;
      if ((strips > 0x7fffffffu) || (bands > 65535u))
        return fail(MH_UNSUPPORTED,"AdaptiveThresholdImage: %zux%zu frame is outside the launch grid",src.columns,
          src.rows);
      *grid=dim3((unsigned) strips,(unsigned) bands);
    }
  else
    {
      if ((width > (size_t) kAdaptiveFloatMaxSide) || (height > (size_t) kAdaptiveFloatMaxSide))
        return fail(MH_UNSUPPORTED,"AdaptiveThresholdImage: a %zux%zu window (float Quantum: at most %lld a side)",
          width,height,kAdaptiveFloatMaxSide);
      const size_t chains=src.rows*(size_t) src.channels;
      *grid=dim3((unsigned) ((chains+kAdaptiveFloatThreads-1)/kAdaptiveFloatThreads));
    }
  a->width=(int) width;
  a->height=(int) height;
  a->number_pixels=(double) ((unsigned long long) width*(unsigned long long) height);
  return MH_OK;
}

MhStatus adaptive_threshold_check(const View &src,size_t width,size_t height)
{
  AdaptiveArgs a={};
  dim3 grid;
  return adaptive_plan(src,width,height,&a,&grid);
}

MhStatus launch_adaptive_threshold(const View &src,const View &dst,size_t width,size_t height,double bias,
  uint32_t copy_mask)
{
  AdaptiveArgs a={};
  dim3 grid;
  MH_TRY(adaptive_plan(src,width,height,&a,&grid));
  if ((src.columns == 0) || (src.rows == 0))
    return MH_OK;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.bias=bias;
  a.copy_mask=copy_mask;
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    if constexpr (QuantumOps<Q>::is_float)
      {
        ProfileScope prof("adaptive_threshold_float",src.stream);
        hipLaunchKernelGGL((adaptive_float_kernel<Q,L.C>),grid,dim3(kAdaptiveFloatThreads),0,src.stream,a);
        MH_HIP(hipGetLastError());
      }
    else
      {
        ProfileScope prof("adaptive_threshold_q16",src.stream);
        hipLaunchKernelGGL((adaptive_q16_kernel<Q,L.C>),grid,dim3(kAdaptiveThreads),0,src.stream,a);
        MH_HIP(hipGetLastError());
      }
    return MhStatus(MH_OK);
  });
}

} // namespace mh
