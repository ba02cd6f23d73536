// SampleImage and ScaleImage of MagickCore/resize.c on the device.
//
//   SampleImage :3907-4075    a gather: destination (x,y) takes every defined channel of source
//                             (x_offset[x], y_offset[y]) verbatim; the two tables come from the host
//   ScaleImage :4106-4536     the host plan (scale_plan.hpp) lists, per destination row and per
//                             destination column, the ordered (source, weight) terms of the reference's
//                             running sums.  Per sample:  premultiply (alpha*p on channels with the Blend
//                             trait, alpha = QuantumScale*alpha sample), the row terms into an fp64
//                             scanline, the column terms over that scanline, PerceptibleReciprocal of the
//                             scaled alpha, ClampToQuantum.  Every sum starts from 0.0 and every multiply
//                             and add is rounded separately, in the plan's order (0.0+x is not x for
//                             x = -0.0, which float Quantum would store).  An axis with equal source and
//                             destination does no arithmetic.  No libm: bit-identical in both modes.
//
// MI355X mapping:
//   scale_fused_kernel       one workgroup per destination row and run of kScaleThreads (or fewer)
//                            destination columns.  A lane per source column of the run's source interval
//                            forms the row sum in registers (coalesced row reads, kScaleBatch rows in flight,
//                            the weight a scalar) and
//                            puts it in LDS; after one barrier a lane per destination column walks its
//                            column terms out of LDS and stores the pixel.  The fp64 scanline never
//                            reaches memory.  Taken when both axes' longest term list has at most
//                            kScaleFusedTerms entries and the interval fits kScaleLdsBytes.
//   scale_rows_kernel + scale_columns_kernel   the generic form, any geometry: the fp64 scanlines of
//                            all destination rows in a temp-pool block, one lane per sample each.
//   sample_kernel            one lane per destination pixel
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "scale_plan.hpp"

#include <algorithm>

namespace mh {

constexpr int kScaleThreads=256;
constexpr size_t kScaleFusedTerms=64;             // longest term list the one-launch kernel takes
constexpr size_t kScaleLdsBytes=65536;            // its staged scanline interval: [columns][C] doubles
constexpr int kScaleMinRun=32;                    // shortest run of destination columns per workgroup

struct ScaleArgs
{
  const void *src;
  void *dst;
  double *scanlines;                              // generic form: [destination rows][source columns][C]
  int src_columns,src_rows,dst_columns,dst_rows;
  const uint32_t *row_start,*column_start;        // destination+1 entries each; unused on an identity axis
  const int32_t *row_index,*column_index;
  const double *row_weight,*column_weight;
  int rows_identity,columns_identity;
  uint32_t blend_mask,store_mask;
  int alpha;                                      // offset of alpha, -1: none
  int run,runs;                                   // fused: destination columns per workgroup, workgroups per row
  int interval;                                   // fused: capacity of the staged interval, source columns
};

constexpr int kScaleBatch=4;                      // terms whose loads are issued together

// x_vector of one source pixel, resize.c:4239-4260
template<typename Q,int C>
static __device__ __forceinline__ void scale_premultiplied(const ScaleArgs &a,const Q (&q)[C],double (&x)[C])
{
  double alpha=1.0;
  if (a.alpha >= 0)
    alpha=kQS*(double) q[a.alpha < C ? a.alpha : C-1];
#pragma unroll
  for (int c=0; c < C; c++)
    x[c]=((a.blend_mask >> c) & 1u) != 0 ? alpha*(double) q[c] : (double) q[c];
}

// scanline[column] of destination row y, resize.c:4227-4372
template<typename Q,int C>
static __device__ __forceinline__ void scale_row_sum(const ScaleArgs &a,int y,int column,double (&sum)[C])
{
  const Q *src=static_cast<const Q *>(a.src);
  if (a.rows_identity != 0)
    {
      Q q[C];
      load_pixel<Q,C>(src+((size_t) y*(size_t) a.src_columns+(size_t) column)*C,q);
      scale_premultiplied<Q,C>(a,q,sum);
      return;
    }
#pragma unroll
  for (int c=0; c < C; c++)
    sum[c]=0.0;
  const uint32_t last=a.row_start[y+1];
  uint32_t k=a.row_start[y];
  // a reduction's list is long and its loads do not depend on one another: kScaleBatch rows are in
  // flight at a time; the sums keep the list's order
  for (; k+kScaleBatch <= last; k+=kScaleBatch)
    {
      Q q[kScaleBatch][C];
#pragma unroll
      for (int j=0; j < kScaleBatch; j++)
        load_pixel<Q,C>(src+((size_t) a.row_index[k+j]*(size_t) a.src_columns+(size_t) column)*C,q[j]);
#pragma unroll
      for (int j=0; j < kScaleBatch; j++)
        {
          const double weight=a.row_weight[k+j];
          double x[C];
          scale_premultiplied<Q,C>(a,q[j],x);
#pragma unroll
          for (int c=0; c < C; c++)
            sum[c]=sum[c]+weight*x[c];
        }
    }
  for (; k < last; k++)
    {
      const double weight=a.row_weight[k];
      Q q[C];
      load_pixel<Q,C>(src+((size_t) a.row_index[k]*(size_t) a.src_columns+(size_t) column)*C,q);
      double x[C];
      scale_premultiplied<Q,C>(a,q,x);
#pragma unroll
      for (int c=0; c < C; c++)
        sum[c]=sum[c]+weight*x[c];
    }
}

// resize.c:4378-4409, :4475-4507: the scaled sums of one destination pixel to Quanta
template<typename Q,int C>
static __device__ __forceinline__ void scale_store(const ScaleArgs &a,int y,int d,const double (&sum)[C])
{
  Q *out=static_cast<Q *>(a.dst)+((size_t) y*(size_t) a.dst_columns+(size_t) d)*C;
  Q q[C];
  if (a.store_mask != ((1u << C)-1u))
    load_pixel<Q,C>(out,q);
  double alpha=1.0;
  if (a.alpha >= 0)
    alpha=perceptible_reciprocal(kQS*sum[a.alpha < C ? a.alpha : C-1]);
#pragma unroll
  for (int c=0; c < C; c++)
    if (((a.store_mask >> c) & 1u) != 0)
      q[c]=QuantumOps<Q>::clamp(((a.blend_mask >> c) & 1u) != 0 ? alpha*sum[c] : sum[c]);
  store_pixel<Q,C>(out,q);
}

// first and last source column the destination columns [d0, d1) read
static __device__ __forceinline__ void scale_interval(const ScaleArgs &a,int d0,int d1,int &low,int &high)
{
  if (a.columns_identity != 0)
    {
      low=d0;
      high=d1-1;
      return;
    }
  low=a.column_index[a.column_start[d0]];
  high=a.column_index[a.column_start[d1]-1];
}

template<typename Q,int C>
__global__ __launch_bounds__(kScaleThreads)
void scale_fused_kernel(ScaleArgs a)
{
  extern __shared__ double scale_scanline[];       // [interval][C]
  const int y=(int) (blockIdx.x/(unsigned) a.runs);
  const int d0=(int) (blockIdx.x % (unsigned) a.runs)*a.run;
  const int d1=d0+a.run < a.dst_columns ? d0+a.run : a.dst_columns;
  int low,high;
  scale_interval(a,d0,d1,low,high);
  // the launcher sized the interval from the same tables; never write past it
  if (high-low+1 > a.interval)
    high=low+a.interval-1;
  for (int column=low+(int) threadIdx.x; column <= high; column+=kScaleThreads)
    {
      double sum[C];
      scale_row_sum<Q,C>(a,y,column,sum);
#pragma unroll
      for (int c=0; c < C; c++)
        scale_scanline[(size_t) (column-low)*C+c]=sum[c];
    }
  __syncthreads();
  for (int d=d0+(int) threadIdx.x; d < d1; d+=kScaleThreads)
    {
      double sum[C];
      if (a.columns_identity != 0)
        {
#pragma unroll
          for (int c=0; c < C; c++)
            sum[c]=scale_scanline[(size_t) (d-low)*C+c];
        }
      else
        {
#pragma unroll
          for (int c=0; c < C; c++)
            sum[c]=0.0;
          const uint32_t last=a.column_start[d+1];
          uint32_t k=a.column_start[d];
          for (; k+kScaleBatch <= last; k+=kScaleBatch)
            {
              double weight[kScaleBatch];
              int column[kScaleBatch];
#pragma unroll
              for (int j=0; j < kScaleBatch; j++)
                {
                  weight[j]=a.column_weight[k+j];
                  column[j]=a.column_index[k+j]-low;
                  column[j]=column[j] < 0 ? 0 : (column[j] > high-low ? high-low : column[j]);
                }
#pragma unroll
              for (int j=0; j < kScaleBatch; j++)
#pragma unroll
                for (int c=0; c < C; c++)
                  sum[c]=sum[c]+weight[j]*scale_scanline[(size_t) column[j]*C+c];
            }
          for (; k < last; k++)
            {
              const double weight=a.column_weight[k];
              int column=a.column_index[k]-low;
              column=column < 0 ? 0 : (column > high-low ? high-low : column);
#pragma unroll
              for (int c=0; c < C; c++)
                sum[c]=sum[c]+weight*scale_scanline[(size_t) column*C+c];
            }
        }
      scale_store<Q,C>(a,y,d,sum);
    }
}

// generic form, first launch: one lane per (destination row, source column)
template<typename Q,int C>
__global__ __launch_bounds__(kScaleThreads)
void scale_rows_kernel(ScaleArgs a)
{
  const unsigned long long count=(unsigned long long) a.dst_rows*(unsigned long long) a.src_columns;
  const unsigned long long stride=(unsigned long long) gridDim.x*kScaleThreads;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kScaleThreads+threadIdx.x; i < count; i+=stride)
    {
      const int y=(int) (i/(unsigned long long) a.src_columns);
      const int column=(int) (i % (unsigned long long) a.src_columns);
      double sum[C];
      scale_row_sum<Q,C>(a,y,column,sum);
#pragma unroll
      for (int c=0; c < C; c++)
        a.scanlines[i*C+c]=sum[c];
    }
}

// ... second launch: one lane per destination pixel
template<typename Q,int C>
__global__ __launch_bounds__(kScaleThreads)
void scale_columns_kernel(ScaleArgs a)
{
  const unsigned long long count=(unsigned long long) a.dst_rows*(unsigned long long) a.dst_columns;
  const unsigned long long stride=(unsigned long long) gridDim.x*kScaleThreads;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kScaleThreads+threadIdx.x; i < count; i+=stride)
    {
      const int y=(int) (i/(unsigned long long) a.dst_columns);
      const int d=(int) (i % (unsigned long long) a.dst_columns);
      const double *scanline=a.scanlines+(size_t) y*(size_t) a.src_columns*C;
      double sum[C];
      if (a.columns_identity != 0)
        {
#pragma unroll
          for (int c=0; c < C; c++)
            sum[c]=scanline[(size_t) d*C+c];
        }
      else
        {
#pragma unroll
          for (int c=0; c < C; c++)
            sum[c]=0.0;
          const uint32_t last=a.column_start[d+1];
          for (uint32_t k=a.column_start[d]; k < last; k++)
            {
              const double weight=a.column_weight[k];
              const double *s=scanline+(size_t) a.column_index[k]*C;
#pragma unroll
              for (int c=0; c < C; c++)
                sum[c]=sum[c]+weight*s[c];
            }
        }
      scale_store<Q,C>(a,y,d,sum);
    }
}

// ------------------------------------------------------------------ SampleImage
struct SampleArgs
{
  const void *src;
  void *dst;
  int src_columns,dst_columns;
  unsigned long long count;                        // destination pixels
  const long long *x_offset,*y_offset;
  uint32_t store_mask;
};

template<typename Q,int C>
__global__ __launch_bounds__(kScaleThreads)
void sample_kernel(SampleArgs a)
{
  const Q *src=static_cast<const Q *>(a.src);
  Q *dst=static_cast<Q *>(a.dst);
  const unsigned long long stride=(unsigned long long) gridDim.x*kScaleThreads;
  for (unsigned long long i=(unsigned long long) blockIdx.x*kScaleThreads+threadIdx.x; i < a.count; i+=stride)
    {
      const unsigned long long y=i/(unsigned long long) a.dst_columns,x=i % (unsigned long long) a.dst_columns;
      Q p[C];
      load_pixel<Q,C>(src+((size_t) a.y_offset[y]*(size_t) a.src_columns+(size_t) a.x_offset[x])*C,p);
      if (a.store_mask != ((1u << C)-1u))
        {
          Q q[C];
          load_pixel<Q,C>(dst+i*C,q);
#pragma unroll
          for (int c=0; c < C; c++)
            if (((a.store_mask >> c) & 1u) == 0)
              p[c]=q[c];
        }
      store_pixel<Q,C>(dst+i*C,p);
    }
}

// ------------------------------------------------------------------ launchers
static unsigned scale_grid(unsigned long long items)
{
  unsigned long long blocks=(items+kScaleThreads-1)/kScaleThreads;
  blocks=blocks > 16384ull ? 16384ull : blocks;
  return (unsigned) (blocks < 1 ? 1 : blocks);
}

MhStatus launch_sample(const View &src,const View &dst,const long long *x_offset,const long long *y_offset,
  uint32_t store_mask)
{
  if ((src.columns > 0x7fffffffu) || (dst.columns > 0x7fffffffu))
    return fail(MH_UNSUPPORTED,"SampleImage: a frame wider than 2^31-1 columns");
  SampleArgs a={};
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.src_columns=(int) src.columns;
  a.dst_columns=(int) dst.columns;
  a.count=(unsigned long long) dst.columns*(unsigned long long) dst.rows;
  a.x_offset=x_offset;
  a.y_offset=y_offset;
  a.store_mask=store_mask & ((1u << src.channels)-1u);
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    ProfileScope prof("sample",dst.stream);
    hipLaunchKernelGGL((sample_kernel<typename decltype(L)::Q,L.C>),dim3(scale_grid(a.count)),dim3(kScaleThreads),0,
      dst.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

// The longest source interval a run of `run` destination columns reads (what the fused kernel stages).
static size_t scale_longest_interval(const ScaleAxisPlan &columns,size_t run)
{
  size_t longest=0;
  for (size_t d0=0; d0 < columns.destination; d0+=run)
    {
      const size_t d1=std::min(d0+run,columns.destination);
      size_t low=d0,high=d1-1;
      if (!columns.identity)
        {
          low=(size_t) columns.index[columns.start[d0]];
          high=(size_t) columns.index[columns.start[d1]-1];
        }
      longest=std::max(longest,high-low+1);
    }
  return longest;
}

MhStatus launch_scale(const View &src,const View &dst,const ScalePlan &plan,uint32_t blend_mask,
  uint32_t store_mask,int alpha)
{
  if (!plan.rows.valid || !plan.columns.valid)
    return fail(MH_UNSUPPORTED,"ScaleImage: no plan for %zux%zu -> %zux%zu",src.columns,src.rows,dst.columns,dst.rows);
  if ((src.columns > 0x3fffffffu) || (src.rows > 0x3fffffffu) || (dst.columns > 0x3fffffffu) || (dst.rows > 0x3fffffffu))
    return fail(MH_UNSUPPORTED,"ScaleImage: a frame side above 2^30");
  const int C=src.channels;
  ScaleArgs a={};
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.src_columns=(int) src.columns;
  a.src_rows=(int) src.rows;
  a.dst_columns=(int) dst.columns;
  a.dst_rows=(int) dst.rows;
  a.rows_identity=plan.rows.identity ? 1 : 0;
  a.columns_identity=plan.columns.identity ? 1 : 0;
  a.blend_mask=alpha >= 0 ? blend_mask & ((1u << C)-1u) : 0u;
  a.store_mask=store_mask & ((1u << C)-1u);
  a.alpha=(alpha >= 0) && (alpha < C) ? alpha : -1;
  // the six tables as one block and one copy
  TableBundle tables;
  static const uint32_t no_start[2]={0u,0u};
  static const int32_t no_index[1]={0};
  static const double no_weight[1]={0.0};
  const auto add=[&](const ScaleAxisPlan &axis,size_t (&slot)[3])
  {
    const bool empty=axis.identity || axis.index.empty();
    slot[0]=tables.add(empty ? (const void *) no_start : axis.start.data(),empty ? sizeof(no_start) : axis.start.size()*sizeof(uint32_t));
    slot[1]=tables.add(empty ? (const void *) no_index : axis.index.data(),empty ? sizeof(no_index) : axis.index.size()*sizeof(int32_t));
    slot[2]=tables.add(empty ? (const void *) no_weight : axis.weight.data(),empty ? sizeof(no_weight) : axis.weight.size()*sizeof(double));
  };
  size_t row_slot[3],column_slot[3];
  add(plan.rows,row_slot);
  add(plan.columns,column_slot);
  MH_TRY(tables.upload(src.device,src.stream));
  a.row_start=tables.at<uint32_t>(row_slot[0]);
  a.row_index=tables.at<int32_t>(row_slot[1]);
  a.row_weight=tables.at<double>(row_slot[2]);
  a.column_start=tables.at<uint32_t>(column_slot[0]);
  a.column_index=tables.at<int32_t>(column_slot[1]);
  a.column_weight=tables.at<double>(column_slot[2]);

  // one launch: the longest run of destination columns whose source interval fits the LDS budget
  int run=0;
  size_t interval=0;
  if ((plan.rows.longest <= kScaleFusedTerms) && (plan.columns.longest <= kScaleFusedTerms))
    for (int candidate=kScaleThreads; candidate >= kScaleMinRun; candidate/=2)
      {
        interval=scale_longest_interval(plan.columns,(size_t) candidate);
        if (interval*(size_t) C*sizeof(double) <= kScaleLdsBytes)
          {
            run=candidate;
            break;
          }
      }
  const unsigned long long runs=run > 0 ? (dst.columns+(size_t) run-1)/(size_t) run : 0;
  if ((run > 0) && (runs*(unsigned long long) dst.rows <= 0x7fffffffull))
    {
      a.run=run;
      a.runs=(int) runs;
      a.interval=(int) interval;
      const size_t lds=interval*(size_t) C*sizeof(double);
      return dispatch_layout(src.quantum,C,[&](auto L) {
        ProfileScope prof("scale_fused",dst.stream);
        hipLaunchKernelGGL((scale_fused_kernel<typename decltype(L)::Q,L.C>),dim3((unsigned) (runs*dst.rows)),
          dim3(kScaleThreads),lds,dst.stream,a);
        MH_HIP(hipGetLastError());
        return MhStatus(MH_OK);
      });
    }
  // any geometry: the fp64 scanlines through memory
  Temp scanlines;
  MH_TRY(scanlines.alloc(src.device,dst.rows*src.columns*(size_t) C*sizeof(double),src.stream));
  a.scanlines=scanlines.as<double>();
  return dispatch_layout(src.quantum,C,[&](auto L) {
    using Q=typename decltype(L)::Q;
    {
      ProfileScope prof("scale_rows",dst.stream);
      hipLaunchKernelGGL((scale_rows_kernel<Q,L.C>),dim3(scale_grid((unsigned long long) dst.rows*src.columns)),
        dim3(kScaleThreads),0,dst.stream,a);
      MH_HIP(hipGetLastError());
    }
    ProfileScope prof("scale_columns",dst.stream);
    hipLaunchKernelGGL((scale_columns_kernel<Q,L.C>),dim3(scale_grid((unsigned long long) dst.rows*dst.columns)),
      dim3(kScaleThreads),0,dst.stream,a);
    MH_HIP(hipGetLastError());
    return MhStatus(MH_OK);
  });
}

} // namespace mh
