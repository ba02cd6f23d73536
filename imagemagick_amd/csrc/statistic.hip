// StatisticImage (MagickCore/statistic.c:2918-3163): every output sample is a statistic of the
// W x H window whose top-left corner is (x - W/2, y - H/2), W = max(width,1), H = max(height,1),
// edge-clamped outside the frame.  Every channel of the update mask on its own (no alpha
// weighting); copy channels take the source sample at the window centre.
//
// MI355X mapping: a workgroup of 256 lanes computes a 16 x 16 block of
// outputs.  Channel by channel it stages the block's (15+W) x (15+H) edge-clamped window in LDS,
// then every lane reads its own window from there.  Five routes, chosen by the window and the
// type only:
//   statistic_rank_net16   median / mode / nonpeak, n = W*H <= 16: the n 16-bit keys in registers
//   statistic_rank_net32   ... 16 < n <= 32: sorted by Batcher's odd-even merge network, then
//                          median, mode and nonpeak read off the sorted registers
//   statistic_rank_select  ... n > 32: a radix-4 selection of the median key over the LDS window
//                          (8 counting passes), one more pass for nonpeak's neighbours; mode
//                          walks the distinct keys in ascending order with their counts
//   statistic_extreme      minimum / maximum / gradient / contrast: a raster-order scan of the
//                          raw samples (the reference's own order, so NaN behaves alike)
//   statistic_moment       mean / RMS / standard deviation: exact integer sums on Q16, fp64
//                          sums in the reference's raster order on float Quantum (no FMA)
// The rank routes stage ScaleQuantumToShort keys (quantum-private.h:517-528) as 16-bit LDS
// words, so Q16 and float Quantum share one selection code path; the other two stage raw Quantum.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"

#include <algorithm>
#include <type_traits>

namespace mh {

// MhStatisticType (statistic.h:139-152)
enum
{
  ST_UNDEFINED=0,ST_GRADIENT=1,ST_MAXIMUM=2,ST_MEAN=3,ST_MEDIAN=4,ST_MINIMUM=5,ST_MODE=6,ST_NONPEAK=7,
  ST_RMS=8,ST_STDDEV=9,ST_CONTRAST=10
};

enum StatRoute { SR_NET16=0,SR_NET32=1,SR_SELECT=2,SR_EXTREME=3,SR_MOMENT=4 };

constexpr int kStatBlock=kWindowBlock;       // outputs per workgroup: kStatBlock x kStatBlock
constexpr size_t kStatMaxLds=65536;          // bytes of one staged channel window

struct StatArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int width,height;          // W, H >= 1
  int tile_w,tile_h;         // kStatBlock-1+W, kStatBlock-1+H
  int type;
  uint32_t copy_mask;
};

// ScaleQuantumToShort: Q16 the sample itself; float Quantum NaN / <= 0 -> 0, >= 65535 -> 65535,
// else (unsigned short) (q+0.5f) with the add in f32
static __device__ __forceinline__ uint16_t stat_key(uint16_t q) { return q; }
static __device__ __forceinline__ uint16_t stat_key(float q)
{
  if (!(q > 0.0f))
    return 0;
  if (q >= 65535.0f)
    return 65535;
  return (uint16_t) __fadd_rn(q,0.5f);
}

template<typename Q,typename T,bool KEYS>
static __device__ __forceinline__ T stat_stage_value(Q q)
{
  if constexpr (KEYS)
    return (T) stat_key(q);
  else
    return (T) q;
}

// Batcher's odd-even merge sort of N (a power of two) registers, ascending; every index is a
// compile-time constant once the loops are unrolled
template<int N>
static __device__ __forceinline__ void stat_sort(unsigned (&k)[N])
{
#pragma unroll
  for (int p=1; p < N; p<<=1)
#pragma unroll
    for (int q=p; q >= 1; q>>=1)
#pragma unroll
      for (int j=q % p; j <= N-1-q; j+=2*q)
#pragma unroll
        for (int i=0; i < q; i++)
          if ((i+j+q < N) && ((i+j)/(2*p) == (i+j+q)/(2*p)))
            {
              const unsigned a=k[i+j],b=k[i+j+q];
              k[i+j]=a < b ? a : b;
              k[i+j+q]=a < b ? b : a;
            }
}

// median / mode / nonpeak of the n (<= N) keys of the window at `t` (row pitch tile_w)
template<int N>
static __device__ __forceinline__ unsigned stat_rank_net(const uint16_t *t,int tile_w,int W,int n,int type)
{
  unsigned k[N];
  int u=0,v=0;
#pragma unroll
  for (int i=0; i < N; i++)
    {
      k[i]=i < n ? (unsigned) t[v*tile_w+u] : 0x10000u;     // padding sorts behind every key
      if (++u == W)
        {
          u=0;
          v++;
        }
    }
  stat_sort<N>(k);
  const int half=n >> 1;
  unsigned median=k[0];
#pragma unroll
  for (int i=1; i < N; i++)
    median=i == half ? k[i] : median;
  if (type == ST_MODE)
    {
      // GetModePixelList: the lowest key with the largest count (strict >, from a count of 0)
      unsigned mode=k[0],best=0,run=0;
#pragma unroll
      for (int i=0; i < N; i++)
        if (i < n)
          {
            run=((i > 0) && (k[i] == k[i-1])) ? run+1 : 1;
            if (run > best)
              {
                best=run;
                mode=k[i];
              }
          }
      return mode;
    }
  if (type == ST_NONPEAK)
    {
      // GetNonpeakPixelList: the median's neighbours in the list of distinct keys
      unsigned below=0x10000u,above=0x10000u,largest=k[0];
#pragma unroll
      for (int i=0; i < N; i++)
        if (i < n)
          {
            below=k[i] < median ? k[i] : below;
            above=((k[i] > median) && (above == 0x10000u)) ? k[i] : above;
            largest=k[i];
          }
      const bool smaller=k[0] < median,larger=largest > median;
      if (!smaller && larger)
        return above;
      if (smaller && !larger)
        return below;
      return median;
    }
  return median;
}

// n > 32: selection over the staged window
static __device__ __forceinline__ unsigned stat_rank_select(const uint16_t *t,int tile_w,int W,int H,int type)
{
  const int n=W*H;
  if (type == ST_MODE)
    {
      // the distinct keys in ascending order with their counts; stops once the samples left
      // cannot outnumber the best count
      int current=-1,taken=0;
      unsigned mode=0,best=0;
      while ((taken < n) && ((unsigned) (n-taken) > best))
        {
          unsigned next=0x10000u,count=0;
          for (int v=0; v < H; v++)
            {
              const uint16_t *row=t+v*tile_w;
              for (int u=0; u < W; u++)
                {
                  const unsigned key=row[u];
                  if ((int) key > current)
                    {
                      count=key == next ? count+1 : (key < next ? 1u : count);
                      next=key < next ? key : next;
                    }
                }
            }
          if (count > best)
            {
              best=count;
              mode=next;
            }
          taken+=(int) count;
          current=(int) next;
        }
      return mode;
    }
  // the key of rank n>>1, two bits a pass: counts of the three lower digits under the prefix
  unsigned rank=(unsigned) (n >> 1),prefix=0;
  for (int shift=14; shift >= 0; shift-=2)
    {
      const unsigned base=prefix >> shift;
      unsigned c0=0,c1=0,c2=0;
      for (int v=0; v < H; v++)
        {
          const uint16_t *row=t+v*tile_w;
          for (int u=0; u < W; u++)
            {
              const unsigned digit=((unsigned) row[u] >> shift)-base;
              c0+=digit == 0u ? 1u : 0u;
              c1+=digit == 1u ? 1u : 0u;
              c2+=digit == 2u ? 1u : 0u;
            }
        }
      unsigned d=0;
      if (rank >= c0)
        {
          rank-=c0;
          d=1;
          if (rank >= c1)
            {
              rank-=c1;
              d=2;
              if (rank >= c2)
                {
                  rank-=c2;
                  d=3;
                }
            }
        }
      prefix|=d << shift;
    }
  const unsigned median=prefix;
  if (type != ST_NONPEAK)
    return median;
  int below=-1;
  unsigned above=0x10000u;
  for (int v=0; v < H; v++)
    {
      const uint16_t *row=t+v*tile_w;
      for (int u=0; u < W; u++)
        {
          const unsigned key=row[u];
          below=(key < median) && ((int) key > below) ? (int) key : below;
          above=(key > median) && (key < above) ? key : above;
        }
    }
  const bool smaller=below >= 0,larger=above != 0x10000u;
  if (!smaller && larger)
    return above;
  if (smaller && !larger)
    return (unsigned) below;
  return median;
}

// minimum / maximum / gradient / contrast over the raw samples, raster order from the first one
template<typename Q>
static __device__ __forceinline__ Q stat_extreme(const Q *t,int tile_w,int W,int H,int type)
{
  Q minimum=t[0],maximum=t[0];
  for (int v=0; v < H; v++)
    {
      const Q *row=t+v*tile_w;
      for (int u=0; u < W; u++)
        {
          const Q s=row[u];
          minimum=s < minimum ? s : minimum;
          maximum=s > maximum ? s : maximum;
        }
    }
  const double lo=(double) minimum,hi=(double) maximum;
  double r;
  switch (type)
  {
    case ST_MINIMUM: r=lo; break;
    case ST_MAXIMUM: r=hi; break;
    case ST_GRADIENT: r=hi-lo; break;
    default: r=(hi-lo)*perceptible_reciprocal(hi+lo); break;        // ST_CONTRAST
  }
  // MagickAbsoluteValue (image-private.h:45) is a comparison, not fabs: -0.0 stays -0.0.  A float window of equal
  // negative samples has the contrast 0.0*(1/(2*sample)) = -0.0
  if (((type == ST_GRADIENT) || (type == ST_CONTRAST)) && (r < 0.0))
    r=-r;
  return QuantumOps<Q>::clamp(r);
}

// mean / RMS / standard deviation: Q16 sums are exact integers (n*65535^2 < 2^53), float Quantum
// sums are fp64 in the reference's order, rows outer, columns inner
template<typename Q>
static __device__ __forceinline__ Q stat_moment(const Q *t,int tile_w,int W,int H,int type)
{
  double sum,sum_squared;
  if constexpr (QuantumOps<Q>::is_float)
    {
      sum=0.0;
      sum_squared=0.0;
      for (int v=0; v < H; v++)
        {
          const Q *row=t+v*tile_w;
          for (int u=0; u < W; u++)
            {
              const double s=(double) row[u];
              sum=__dadd_rn(sum,s);
              sum_squared=__dadd_rn(sum_squared,__dmul_rn(s,s));
            }
        }
    }
  else
    {
      unsigned long long s1=0,s2=0;
      for (int v=0; v < H; v++)
        {
          const Q *row=t+v*tile_w;
          unsigned r1=0;
          unsigned long long r2=0;
          for (int u=0; u < W; u++)
            {
              const unsigned s=row[u];
              r1+=s;
              r2+=(unsigned long long) (s*s);
            }
          s1+=r1;
          s2+=r2;
        }
      sum=(double) s1;
      sum_squared=(double) s2;
    }
  const double area=(double) W*(double) H;
  double r;
  switch (type)
  {
    case ST_RMS: r=sqrt(sum_squared/area); break;
    case ST_STDDEV: r=sqrt(sum_squared/area-(sum/area*sum/area)); break;
    default: r=sum/area; break;                                           // ST_MEAN, ST_UNDEFINED
  }
  return QuantumOps<Q>::clamp(r);
}

template<typename Q,int C,int ROUTE>
__global__ __launch_bounds__(256)
void statistic_kernel(StatArgs a)
{
  constexpr bool kKeys=ROUTE <= SR_SELECT;
  using T=typename std::conditional<kKeys,uint16_t,Q>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char stat_smem[];
  T *tile=reinterpret_cast<T *>(stat_smem);
  const Q *src=static_cast<const Q *>(a.src);
  const int tx=(int) (threadIdx.x % kStatBlock),ty=(int) (threadIdx.x/kStatBlock);
  const int x0=(int) blockIdx.x*kStatBlock,y0=(int) blockIdx.y*kStatBlock;
  const int x=x0+tx,y=y0+ty;
  const bool inside=(x < a.columns) && (y < a.rows);
  const int left=x0-a.width/2,top=y0-a.height/2;
  const int area=a.tile_w*a.tile_h;
  Q out[C];
  if (inside)
    load_pixel<Q,C>(src+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.copy_mask >> c) & 1u)
        continue;                                   // the source sample at the window centre
      __syncthreads();                              // the previous channel's readers are done
      for (int i=(int) threadIdx.x; i < area; i+=(int) blockDim.x)
        {
          const int r=i/a.tile_w,col=i-r*a.tile_w;
          const int gx=min(max(left+col,0),a.columns-1),gy=min(max(top+r,0),a.rows-1);
          tile[i]=stat_stage_value<Q,T,kKeys>(src[((size_t) gy*(size_t) a.columns+(size_t) gx)*C+c]);
        }
      __syncthreads();
      if (!inside)
        continue;
      const T *t=tile+ty*a.tile_w+tx;
      if constexpr (ROUTE == SR_NET16)
        out[c]=(Q) stat_rank_net<16>(t,a.tile_w,a.width,a.width*a.height,a.type);
      else if constexpr (ROUTE == SR_NET32)
        out[c]=(Q) stat_rank_net<32>(t,a.tile_w,a.width,a.width*a.height,a.type);
      else if constexpr (ROUTE == SR_SELECT)
        out[c]=(Q) stat_rank_select(t,a.tile_w,a.width,a.height,a.type);
      else if constexpr (ROUTE == SR_EXTREME)
        out[c]=stat_extreme<Q>(t,a.tile_w,a.width,a.height,a.type);
      else
        out[c]=stat_moment<Q>(t,a.tile_w,a.width,a.height,a.type);
    }
  if (inside)
    store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
}

static const char *const kStatRouteNames[]={"statistic_rank_net16","statistic_rank_net32",
  "statistic_rank_select","statistic_extreme","statistic_moment"};

template<typename Q,int C,int ROUTE>
static MhStatus statistic_launch(const StatArgs &a,size_t lds,hipStream_t stream)
{
  ProfileScope prof(kStatRouteNames[ROUTE],stream);
  hipLaunchKernelGGL((statistic_kernel<Q,C,ROUTE>),window_grid(a.columns,a.rows),dim3(kStatBlock*kStatBlock),lds,
    stream,a);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

template<typename Q,int C>
static MhStatus statistic_route(const StatArgs &a,int route,size_t lds,hipStream_t stream)
{
  switch (route)
  {
    case SR_NET16: return statistic_launch<Q,C,SR_NET16>(a,lds,stream);
    case SR_NET32: return statistic_launch<Q,C,SR_NET32>(a,lds,stream);
    case SR_SELECT: return statistic_launch<Q,C,SR_SELECT>(a,lds,stream);
    case SR_EXTREME: return statistic_launch<Q,C,SR_EXTREME>(a,lds,stream);
    default: return statistic_launch<Q,C,SR_MOMENT>(a,lds,stream);
  }
}

MhStatus launch_statistic(const View &src,const View &dst,int type,size_t width,size_t height,
  const Roles &roles)
{
  if ((type < ST_UNDEFINED) || (type > ST_CONTRAST))
    return fail(MH_BAD_ARGUMENT,"StatisticImage: unknown statistic type %d",type);
  const size_t W=std::max<size_t>(width,1),H=std::max<size_t>(height,1);
  const bool rank=(type == ST_MEDIAN) || (type == ST_MODE) || (type == ST_NONPEAK);
  const bool extreme=(type == ST_MINIMUM) || (type == ST_MAXIMUM) || (type == ST_GRADIENT) ||
    (type == ST_CONTRAST);
  const size_t element=rank ? 2u : (src.quantum == MH_QUANTUM_U16 ? 2u : 4u);
  // the staged window of one channel must fit the LDS budget of a workgroup (header: the limit)
  if ((W > 4096) || (H > 4096) ||
      ((W+kStatBlock-1)*(H+kStatBlock-1)*element > kStatMaxLds))
    return fail(MH_UNSUPPORTED,"StatisticImage: a %zux%zu window does not fit the LDS tile",W,H);
  MH_TRY(window_grid_check("StatisticImage",src));
  if ((src.columns == 0) || (src.rows == 0))
    return MH_OK;
  const size_t n=W*H;
  const int route=rank ? (n <= 16 ? SR_NET16 : (n <= 32 ? SR_NET32 : SR_SELECT)) :
    (extreme ? SR_EXTREME : SR_MOMENT);
  StatArgs a;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.width=(int) W;
  a.height=(int) H;
  a.tile_w=(int) W+kStatBlock-1;
  a.tile_h=(int) H+kStatBlock-1;
  a.type=type;
  a.copy_mask=roles.copy_mask;
  const size_t lds=((size_t) a.tile_w*(size_t) a.tile_h*element+15u) & ~(size_t) 15u;
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return statistic_route<typename decltype(L)::Q,L.C>(a,route,lds,src.stream); });
}

} // namespace mh
