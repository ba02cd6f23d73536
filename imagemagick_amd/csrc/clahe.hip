// CLAHEImage (MagickCore/enhance.c:295-785) between its two colourspace transforms: contrast-limited
// adaptive histogram equalisation of channel 0 (L of a Lab frame), bit-identical to the reference on
// Q16 and float Quantum.  The caller (operators_enhance.cpp) runs the exact conversions around it.
//
//   The frame is padded up to whole tw x th tiles, pad_x>>1 columns on the left and pad_y>>1 rows on
//   top, by edge replication.  No padded plane exists here: padded (px,py) reads the frame at
//   (clamp(px-left), clamp(py-top)).  Every sample goes through ScaleQuantumToShort
//   (quantum-private.h:517-528) and lut[v] = v/delta, delta = 65535/bins+1.  Per tile: the
//   histogram of lut[] over the padded tile, ClipCLAHEHistogram with limit =
//   max(1,(size_t) (clip_limit*(tw*th)/bins)), MapCLAHEHistogram.  Then (tiles_x+1) x (tiles_y+1)
//   regions, the border ones tw>>1 / (tw+1)>>1 wide (th likewise), interpolate bilinearly between
//   the four neighbouring tile maps.
//
// MI355X mapping, three launches:
//   clahe_histogram_kernel    `parts` workgroups per tile, each bins a run of the tile's pixels into
//                             256 LDS counters; lanes of a wave that agree on the bin fold into one LDS
//                             atomic (a constant frame: one per wave instead of 64 on one address);
//                             the non-zero counters merge into a zeroed global table with vector atomics
//   clahe_map_kernel          one workgroup per tile, one lane per bin: the two clip loops as per-bin
//                             work plus a reduction; the redistribution's full sweeps (excess >= bins:
//                             stride 1, every bin below the limit gains one) k at a time, the rest by
//                             one lane walking the LDS words statement for statement; integer prefix
//                             sum; one fp64 multiply per bin; uint16 maps out
//   clahe_interpolate_kernel  a workgroup takes a run of one region's pixels, stages the region's four
//                             maps in LDS, forms the weighted sum in 64-bit integers, converts once and
//                             multiplies by the region's reciprocal (from the host: no device division)
// All counts are integers, so their order does not matter; the two fp64 products are single
// operations (-ffp-contract=off, nothing to contract).
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"

#include <algorithm>

namespace mh {

constexpr int kClaheThreads=256;          // lanes per workgroup = the most bins
constexpr int kClaheMaxBins=256;
constexpr unsigned kClaheRun=16384;       // pixels of a tile one histogram workgroup bins
constexpr unsigned kClaheBlock=2048;      // pixels of a region one interpolation workgroup maps

struct ClaheArgs
{
  void *pixels;
  int columns,rows;          // the frame
  int tw,th;                 // tile
  int tiles_x,tiles_y;
  int left,top;              // padding in front of the frame: pad_x>>1, pad_y>>1
  int bins;
  unsigned magic;            // v/delta == umulhi(v,magic) for v < 65536
  unsigned parts;            // histogram workgroups per tile
  unsigned blocks;           // interpolation workgroups per region
  long long limit;           // ClipCLAHEHistogram's clip_limit, an integer
  double scale;              // 65535.0/(tw*th)
  double reciprocal[9];      // PerceptibleReciprocal(width*height) of a region: [3*row kind+column kind]
  uint32_t *counts;          // [tiles][bins]
  uint16_t *maps;            // [tiles][bins]
  int passthrough;           // clip_limit == 1.0: ScaleShortToQuantum(ScaleQuantumToShort()) alone
};

// one count into an LDS histogram; every lane of the wave calls this together
static __device__ __forceinline__ void clahe_count(uint32_t *histogram,unsigned bin,bool valid)
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
  // neighbouring pixels share bins: one atomic per distinct bin, by leader election
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

template<typename Q,int C>
__global__ __launch_bounds__(kClaheThreads)
void clahe_histogram_kernel(ClaheArgs a)
{
  __shared__ uint32_t histogram[kClaheMaxBins];
  const unsigned tile=blockIdx.x/a.parts,part=blockIdx.x-tile*a.parts;
  const int ty=(int) (tile/(unsigned) a.tiles_x),tx=(int) (tile-(unsigned) ty*(unsigned) a.tiles_x);
  histogram[threadIdx.x]=0u;
  __syncthreads();
  const size_t area=(size_t) a.tw*(size_t) a.th;
  const size_t run=(area+a.parts-1)/a.parts;
  const size_t begin=(size_t) part*run,end=begin+run < area ? begin+run : area;
  // (r,c) of this lane's first pixel, then advanced by a workgroup's worth of pixels at a time
  size_t i=begin+threadIdx.x;
  unsigned r=(unsigned) (i/(size_t) a.tw),c=(unsigned) (i-(size_t) r*(size_t) a.tw);
  const unsigned dr=kClaheThreads/(unsigned) a.tw,dc=kClaheThreads-dr*(unsigned) a.tw;
  const Q *pixels=static_cast<const Q *>(a.pixels);
  const size_t rounds=begin < end ? (end-begin+kClaheThreads-1)/kClaheThreads : 0;
  for (size_t k=0; k < rounds; k++,i+=kClaheThreads)
    {
      const bool valid=i < end;
      unsigned bin=0u;
      if (valid)
        {
          const int x=min(max(tx*a.tw+(int) c-a.left,0),a.columns-1);
          const int y=min(max(ty*a.th+(int) r-a.top,0),a.rows-1);
          const Q q=pixels[((size_t) y*(size_t) a.columns+(size_t) x)*C];
          bin=__umulhi(QuantumOps<Q>::map_index(q),a.magic);
        }
      clahe_count(histogram,bin,valid);
      r+=dr;
      c+=dc;
      if (c >= (unsigned) a.tw)
        {
          c-=(unsigned) a.tw;
          r++;
        }
    }
  __syncthreads();
  const uint32_t count=histogram[threadIdx.x];
  if (((int) threadIdx.x < a.bins) && (count != 0u))
    atomicAdd(a.counts+(size_t) tile*(size_t) a.bins+threadIdx.x,count);
}

// sum / minimum over the workgroup; every lane gets the result.  `slots`: four LDS words.
static __device__ __forceinline__ long long clahe_block_sum(long long v,long long *slots)
{
#pragma unroll
  for (int off=32; off > 0; off>>=1)
    v+=__shfl_xor(v,off,64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    slots[threadIdx.x >> 6]=v;
  __syncthreads();
  return slots[0]+slots[1]+slots[2]+slots[3];
}

static __device__ __forceinline__ long long clahe_block_min(long long v,long long *slots)
{
#pragma unroll
  for (int off=32; off > 0; off>>=1)
    {
      const long long other=__shfl_xor(v,off,64);
      v=other < v ? other : v;
    }
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    slots[threadIdx.x >> 6]=v;
  __syncthreads();
  const long long low=slots[0] < slots[1] ? slots[0] : slots[1];
  const long long high=slots[2] < slots[3] ? slots[2] : slots[3];
  return low < high ? low : high;
}

__global__ __launch_bounds__(kClaheThreads)
void clahe_map_kernel(ClaheArgs a)
{
  __shared__ long long histogram[kClaheMaxBins];
  __shared__ long long slots[4];
  __shared__ long long scan[2][kClaheMaxBins];
  const unsigned tile=blockIdx.x;
  const int b=(int) threadIdx.x;
  const long long bins=a.bins,limit=a.limit;
  const bool mine=b < a.bins;
  long long h=mine ? (long long) a.counts[(size_t) tile*(size_t) a.bins+b] : 0;
  // ClipCLAHEHistogram, first loop: the total excess
  long long cumulative_excess=clahe_block_sum(mine && (h > limit) ? h-limit : 0,slots);
  // second loop: clip, and hand every bin below the limit its share
  const long long step=cumulative_excess/bins,excess=limit-step;
  long long taken=0;
  if (mine)
    {
      if (h > limit)
        h=limit;
      else if (h > excess)
        {
          taken=h-excess;
          h=limit;
        }
      else
        {
          taken=step;
          h+=step;
        }
    }
  cumulative_excess-=clahe_block_sum(taken,slots);
  // third loop.  Each pass of the reference's do-while is one strided sweep from bin 0.  While
  // cumulative_excess >= bins the stride is 1 and the excess cannot run out inside a sweep: every bin
  // below the limit gains one, `open` of them.  k such sweeps in a row are k added to each of those
  // bins, as long as none of them fills up (k <= least room) and the excess stays >= bins in front
  // of each of them ((k-1)*open <= cumulative_excess-bins).
  bool finished=false;
  while (cumulative_excess >= bins)
    {
      const bool below=mine && (h < limit);
      const long long open=clahe_block_sum(below ? 1 : 0,slots);
      if (open == 0)
        {
          finished=true;            // a sweep that moves nothing ends the do-while
          break;
        }
      const long long room=clahe_block_min(below ? limit-h : 0x7fffffffffffffffLL,slots);
      const long long fit=(cumulative_excess-bins)/open+1;
      const long long k=room < fit ? room : fit;
      if (below)
        h+=k;
      cumulative_excess-=k*open;
    }
  histogram[b]=h;
  __syncthreads();
  // ... and the remaining sweeps as the reference writes them, one lane on the LDS words
  if ((b == 0) && !finished)
    {
      long long previous_excess;
      do
        {
          previous_excess=cumulative_excess;
          if (cumulative_excess != 0)
            {
              long long stride=bins/cumulative_excess;
              if (stride < 1)
                stride=1;
              for (long long p=0; (p < bins) && (cumulative_excess != 0); p+=stride)
                if (histogram[p] < limit)
                  {
                    histogram[p]++;
                    cumulative_excess--;
                  }
            }
        } while ((cumulative_excess != 0) && (cumulative_excess < previous_excess));
    }
  __syncthreads();
  // MapCLAHEHistogram: the running sum is one of integers, exact in any order
  scan[0][b]=mine ? histogram[b] : 0;
  __syncthreads();
  int from=0;
  for (int off=1; off < kClaheMaxBins; off<<=1)
    {
      scan[from ^ 1][b]=scan[from][b]+(b >= off ? scan[from][b-off] : 0);
      from^=1;
      __syncthreads();
    }
  if (mine)
    {
      const double sum=(double) scan[from][b];
      unsigned long long value=(unsigned long long) (a.scale*sum);
      if (value > 65535ull)
        value=65535ull;
      a.maps[(size_t) tile*(size_t) a.bins+b]=(uint16_t) value;
    }
}

// region `index` of `tiles`+1 along one axis: its first padded coordinate, its extent, the tiles
// whose maps it reads (enhance.c:544-600) and which of the three extents it has
static __device__ __forceinline__ void clahe_region(int index,int tiles,int tile,int *origin,int *extent,
  int *near,int *far,int *kind)
{
  if (index == 0)
    {
      *origin=0;
      *extent=tile >> 1;
      *near=0;
      *far=0;
      *kind=0;
    }
  else if (index == tiles)
    {
      *origin=(tile >> 1)+(index-1)*tile;
      *extent=(tile+1) >> 1;
      *near=tiles-1;
      *far=tiles-1;
      *kind=2;
    }
  else
    {
      *origin=(tile >> 1)+(index-1)*tile;
      *extent=tile;
      *near=index-1;
      *far=index;
      *kind=1;
    }
}

template<typename Q,int C>
__global__ __launch_bounds__(kClaheThreads)
void clahe_interpolate_kernel(ClaheArgs a)
{
  __shared__ uint16_t maps[4][kClaheMaxBins];        // Q12, Q22, Q11, Q21
  const unsigned region=blockIdx.x/a.blocks,block=blockIdx.x-region*a.blocks;
  const int ry=(int) (region/(unsigned) (a.tiles_x+1)),rx=(int) (region-(unsigned) ry*(unsigned) (a.tiles_x+1));
  int x0,y0,W,H,near_x,far_x,near_y,far_y,kind_x,kind_y;
  clahe_region(rx,a.tiles_x,a.tw,&x0,&W,&near_x,&far_x,&kind_x);
  clahe_region(ry,a.tiles_y,a.th,&y0,&H,&near_y,&far_y,&kind_y);
  const size_t area=(size_t) W*(size_t) H;
  const size_t begin=(size_t) block*kClaheBlock;
  if (begin >= area)
    return;
  const size_t end=begin+kClaheBlock < area ? begin+kClaheBlock : area;
  if (!a.passthrough)
    {
      for (int i=(int) threadIdx.x; i < a.bins; i+=kClaheThreads)
        {
          maps[0][i]=a.maps[((size_t) near_y*(size_t) a.tiles_x+(size_t) near_x)*(size_t) a.bins+i];
          maps[1][i]=a.maps[((size_t) near_y*(size_t) a.tiles_x+(size_t) far_x)*(size_t) a.bins+i];
          maps[2][i]=a.maps[((size_t) far_y*(size_t) a.tiles_x+(size_t) near_x)*(size_t) a.bins+i];
          maps[3][i]=a.maps[((size_t) far_y*(size_t) a.tiles_x+(size_t) far_x)*(size_t) a.bins+i];
        }
      __syncthreads();
    }
  const double reciprocal=a.reciprocal[3*kind_y+kind_x];
  size_t i=begin+threadIdx.x;
  unsigned r=(unsigned) (i/(size_t) W),c=(unsigned) (i-(size_t) r*(size_t) W);
  const unsigned dr=kClaheThreads/(unsigned) W,dc=kClaheThreads-dr*(unsigned) W;
  Q *pixels=static_cast<Q *>(a.pixels);
  for (; i < end; i+=kClaheThreads)
    {
      const int x=x0+(int) c-a.left,y=y0+(int) r-a.top;
      if ((x >= 0) && (x < a.columns) && (y >= 0) && (y < a.rows))     // the padding is not stored
        {
          Q *p=pixels+((size_t) y*(size_t) a.columns+(size_t) x)*C;
          unsigned value=QuantumOps<Q>::map_index(p[0]);
          if (!a.passthrough)
            {
              const unsigned bin=__umulhi(value,a.magic);
              // x and y count down from the region's extent (enhance.c:419-431)
              const long long xw=(long long) W-(long long) c,yw=(long long) H-(long long) r;
              const long long sum=yw*(xw*(long long) maps[0][bin]+((long long) W-xw)*(long long) maps[1][bin])+
                ((long long) H-yw)*(xw*(long long) maps[2][bin]+((long long) W-xw)*(long long) maps[3][bin]);
              value=(unsigned) (reciprocal*(double) sum) & 0xffffu;
            }
          p[0]=(Q) value;                                               // ScaleShortToQuantum
        }
      r+=dr;
      c+=dc;
      if (c >= (unsigned) W)
        {
          c-=(unsigned) W;
          r++;
        }
    }
}

static double clahe_perceptible_reciprocal(double x)
{
  const double sign=x < 0.0 ? -1.0 : 1.0;
  if ((sign*x) >= kMagickEpsilon)
    return 1.0/x;
  return sign/kMagickEpsilon;
}

// The geometry and limits of a call (enhance.c:660-677, :513-515, :732-733); nothing is launched.
static MhStatus clahe_plan(const View &img,size_t width,size_t height,size_t number_bins,double clip_limit,
  ClaheArgs *a,size_t *tiles)
{
  if ((img.channels != 3) && (img.channels != 4))
    return fail(MH_UNSUPPORTED,"CLAHEImage: %d channels (the reference re-lays the pixels out on the way to Lab)",
      img.channels);
  const size_t tw=width == 0 ? img.columns >> 3 : width,th=height == 0 ? img.rows >> 3 : height;
  if ((tw == 0) || (th == 0))
    return fail(MH_BAD_ARGUMENT,"CLAHEImage: a %zux%zu tile on a %zux%zu frame",tw,th,img.columns,img.rows);
  if (number_bins == 1)
    return fail(MH_BAD_ARGUMENT,"CLAHEImage: one bin (the reference's bin width wraps to 0)");
  const size_t bins=number_bins == 0 ? 128 : std::min<size_t>(number_bins,kClaheMaxBins);
  if (!(clip_limit >= 0.0))
    return fail(MH_UNSUPPORTED,"CLAHEImage: clip limit %g",clip_limit);
  if ((img.columns == 0) || (img.rows == 0) || (img.columns > 0x3fffffffu) || (img.rows > 0x3fffffffu) ||
      (tw > 0x3fffffffu) || (th > 0x3fffffffu))
    return fail(MH_UNSUPPORTED,"CLAHEImage: %zux%zu frame, %zux%zu tile",img.columns,img.rows,tw,th);
  const size_t pad_x=(img.columns % tw) != 0 ? tw-(img.columns % tw) : 0;
  const size_t pad_y=(img.rows % th) != 0 ? th-(img.rows % th) : 0;
  const size_t padded_columns=img.columns+pad_x,padded_rows=img.rows+pad_y;
  // a tile is at most the padded frame: its counts fit 32 bits, and so do the kernels' coordinates
  if ((padded_columns > 0x3fffffffu) || (padded_rows > 0x3fffffffu) ||
      (padded_columns*padded_rows >= ((size_t) 1 << 32)))
    return fail(MH_UNSUPPORTED,"CLAHEImage: a padded frame of %zux%zu",padded_columns,padded_rows);
  const size_t tiles_x=padded_columns/tw,tiles_y=padded_rows/th;
  *tiles=tiles_x*tiles_y;
  if ((*tiles)*bins*sizeof(uint16_t) > img.bytes())
    return fail(MH_UNSUPPORTED,"CLAHEImage: %zu tile maps of %zu bins are larger than the frame",*tiles,bins);
  const double limit=clip_limit*(double) (tw*th)/(double) bins;
  if (!(limit < 9007199254740992.0))
    return fail(MH_UNSUPPORTED,"CLAHEImage: clip limit %g",clip_limit);
  a->columns=(int) img.columns;
  a->rows=(int) img.rows;
  a->tw=(int) tw;
  a->th=(int) th;
  a->tiles_x=(int) tiles_x;
  a->tiles_y=(int) tiles_y;
  a->left=(int) (pad_x >> 1);
  a->top=(int) (pad_y >> 1);
  a->bins=(int) bins;
  const unsigned delta=(unsigned) (65535u/bins+1u) & 0xffffu;
  // v/delta for v < 65536 as the high word of v*ceil(2^32/delta): the error term v*(magic*delta-2^32)
  // stays below 2^16*delta <= 2^31 < 2^32
  a->magic=(unsigned) ((((uint64_t) 1 << 32)+delta-1u)/delta);
  a->limit=(long long) (size_t) limit;
  if (a->limit < 1)
    a->limit=1;
  a->scale=65535.0/(double) (tw*th);
  const size_t extent_x[3]={tw >> 1,tw,(tw+1) >> 1},extent_y[3]={th >> 1,th,(th+1) >> 1};
  for (int j=0; j < 3; j++)
    for (int i=0; i < 3; i++)
      a->reciprocal[3*j+i]=clahe_perceptible_reciprocal((double) extent_x[i]*(double) extent_y[j]);
  // histogram workgroups per tile: kClaheRun pixels each, but enough of them to give every CU
  // four workgroups when the tiles are few and large
  const size_t area=tw*th;
  size_t parts=(area+kClaheRun-1)/kClaheRun;
  const size_t wanted=4*(size_t) compute_units(img.device);
  if ((*tiles)*parts < wanted)
    parts=std::min<size_t>((wanted+(*tiles)-1)/(*tiles),(area+4*kClaheThreads-1)/(4*kClaheThreads));
  parts=std::max<size_t>(parts,1);
  const size_t regions=(tiles_x+1)*(tiles_y+1),blocks=(area+kClaheBlock-1)/kClaheBlock;
  if (((*tiles)*parts > 0x7fffffffu) || (regions*blocks > 0x7fffffffu))
    return fail(MH_UNSUPPORTED,"CLAHEImage: %zu tiles are outside the launch grid",*tiles);
  a->parts=(unsigned) parts;
  a->blocks=(unsigned) blocks;
  a->passthrough=clip_limit == 1.0 ? 1 : 0;
  return MH_OK;
}

MhStatus clahe_check(const View &img,size_t width,size_t height,size_t number_bins,double clip_limit)
{
  ClaheArgs a={};
  size_t tiles=0;
  return clahe_plan(img,width,height,number_bins,clip_limit,&a,&tiles);
}

template<typename Q,int C>
static MhStatus clahe_launch(const ClaheArgs &a,size_t tiles,hipStream_t stream)
{
  const size_t regions=((size_t) a.tiles_x+1)*((size_t) a.tiles_y+1);
  if (!a.passthrough)
    {
      {
        ProfileScope prof("clahe_histogram",stream);
        hipLaunchKernelGGL((clahe_histogram_kernel<Q,C>),dim3((unsigned) (tiles*a.parts)),dim3(kClaheThreads),0,stream,a);
        MH_HIP(hipGetLastError());
      }
      {
        ProfileScope prof("clahe_map",stream);
        hipLaunchKernelGGL(clahe_map_kernel,dim3((unsigned) tiles),dim3(kClaheThreads),0,stream,a);
        MH_HIP(hipGetLastError());
      }
    }
  ProfileScope prof("clahe_interpolate",stream);
  hipLaunchKernelGGL((clahe_interpolate_kernel<Q,C>),dim3((unsigned) (regions*a.blocks)),dim3(kClaheThreads),0,stream,a);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_clahe(const View &img,size_t width,size_t height,size_t number_bins,double clip_limit)
{
  ClaheArgs a={};
  size_t tiles=0;
  MH_TRY(clahe_plan(img,width,height,number_bins,clip_limit,&a,&tiles));
  a.pixels=img.pixels;
  // clip_limit == 1.0 (enhance.c:500): no maps; on Q16 the write-back stores what it read
  if (a.passthrough && (img.quantum == MH_QUANTUM_U16))
    return MH_OK;
  Temp counts,maps;
  if (!a.passthrough)
    {
      const size_t cells=tiles*(size_t) a.bins;
      MH_TRY(counts.alloc(img.device,cells*sizeof(uint32_t),img.stream));
      MH_TRY(maps.alloc(img.device,cells*sizeof(uint16_t),img.stream));
      MH_HIP(hipMemsetAsync(counts.ptr,0,cells*sizeof(uint32_t),img.stream));
      a.counts=counts.as<uint32_t>();
      a.maps=maps.as<uint16_t>();
    }
  return dispatch_layout(img.quantum,img.channels,[&](auto L) {
    if constexpr (L.C >= 3)
      return clahe_launch<typename decltype(L)::Q,L.C>(a,tiles,img.stream);
    else
      return fail(MH_UNSUPPORTED,"CLAHEImage: %d channels",img.channels);
  });
}

} // namespace mh
