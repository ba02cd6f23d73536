// Separable (1-D) ConvolveMorphology passes — the BlurImage hot loop.
//
// Reference semantics restated (not ported) from MorphologyPrimitive:
//   horizontal 1 x K kernel  : general row path   MagickCore/morphology.c:2811-2979, 3192-3200
//   vertical   K x 1 kernel  : column fast path   MagickCore/morphology.c:2654-2807
// Both evaluate, per Update channel c of output pixel o along the filter axis,
//     s = bias + sum_{v=0..K-1} [alpha_v] * values[K-1-v] * in(o - origin' + v)
//     out = ClampToQuantum(gamma * s),  gamma = 1/sum(alpha_v*values[..]) for
//     Blend channels, 1 otherwise;  origin' = K-1-origin (reflected kernel)
// with edge-clamped reads (cache.c:2663-2679) and the sum taken in ascending v.
//
// MI355X mapping: the 79-tap sigma=10 blur is VALU-bound, so the
// kernels are register-blocked along the filter axis: each lane owns R
// consecutive outputs, streams the R+K-1 inputs they depend on exactly once,
// and keeps the taps in SGPRs (the tap index depends only on wave-uniform
// loop counters).  The column pass reads rows straight from global memory
// (lane = pixel column => every load is one coalesced 512 B row segment); the
// row pass stages a (64R+K-1)-pixel strip per wavefront in LDS with a
// one-slot-per-R padding that makes the stride-R reads bank-conflict free.
//
// Three walks over that frame: plain, blocked, triangular.  What they share with the folded separable passes of
// convolve_folded.hip — arguments, the triangular walk, launch geometry, the host side — is in conv1d_pass.hpp.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "tie_check.hpp"
#include "conv1d_pass.hpp"
#include <cstdlib>
#include <vector>
#include <type_traits>

namespace mh {

// --------------------------------------------------------------- column pass
template<typename Q,int C,bool BLEND,class A,int R,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_column_kernel(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows,K=args.ntaps;
  // XCD-aware tile order: consecutive workgroup ids land on different XCDs
  // (id % 8), so give each XCD a contiguous range of tiles, y fastest, and
  // vertically adjacent tiles (which share K-1 input rows) meet in one L2.
  const unsigned ntx=(unsigned) ((W+63)/64);
  const unsigned nty=(unsigned) ((H+R*WAVES-1)/(R*WAVES));
  const unsigned total=ntx*nty;
  unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  unsigned tile=(id & 7u)*per+(id >> 3);
  if (tile >= total)
    return;
  const int tx=(int) (tile/nty),ty=(int) (tile%nty);
  const int x=tx*64+lane;
  const int xc=x < W ? x : W-1;
  const int y0=(ty*WAVES+wave)*R;
  if (y0 >= H)
    return;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const T *taps=static_cast<const T *>(args.taps);
  const size_t pitch=(size_t) W*C;

  Acc acc;
  acc.init((T) args.bias);
  const int NJ=R+K-1;
  Q cur[C],nxt[C];
  {
    int yy=y0-args.shift;
    yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
    load_pixel<Q,C>(src+(size_t) yy*pitch+(size_t) xc*C,cur);
  }
  // three loops instead of one with a branch: ramp-up (j < R-1), steady state
  // (every one of the R outputs takes a tap) and ramp-down (j >= K)
  auto fetch_next=[&](int j)
  {
    int yy=y0-args.shift+j+1;
    yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
    load_pixel<Q,C>(src+(size_t) yy*pitch+(size_t) xc*C,nxt);
  };
  auto rotate=[&]()
  {
#pragma unroll
    for (int c=0; c < C; c++)
      cur[c]=nxt[c];
  };
  int j=0;
  const int ramp=(R-1) < NJ ? (R-1) : NJ;
  for ( ; j < ramp; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        {
          int t=j-r;
          if ((t >= 0) && (t < K))
            acc.tap(r,taps[t],in);
        }
      rotate();
    }
  for ( ; j < K; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        acc.tap(r,taps[j-r],in);
      rotate();
    }
  for ( ; j < NJ; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        {
          int t=j-r;
          if ((t >= 0) && (t < K))
            acc.tap(r,taps[t],in);
        }
      rotate();
    }
  unsigned changed=0;
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int y=y0+r;
      if (y < H)
        {
          Q center[C],out[C];
          load_pixel<Q,C>(src+(size_t) y*pitch+(size_t) xc*C,center);
          unsigned ch=acc.finish(r,center,args.copy_mask,out,(T) args.bias);
          if (x < W)
            {
              if (args.unsharp_src != nullptr)
                unsharp_on_the_way_out<Q,C>(args,(size_t) y*W+(size_t) x,out);
              store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
              changed+=ch;
            }
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

// ------------------------------------------------------------------ row pass
template<typename Q,int C,bool BLEND,class A,int R,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_row_kernel(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows,K=args.ntaps;
  const int SEG=64*R;                         // outputs per wave
  const int NS=SEG+K-1;                       // input samples per wave
  const int slots=NS+NS/R+1;
  Q *strip=reinterpret_cast<Q *>(smem_raw)+(size_t) wave*slots*C;

  const unsigned ntx=(unsigned) ((W+SEG-1)/SEG);
  const unsigned nty=(unsigned) ((H+WAVES-1)/WAVES);
  const unsigned total=ntx*nty;
  unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  unsigned tile=(id & 7u)*per+(id >> 3);
  if (tile >= total)
    return;
  const int tx=(int) (tile%ntx),ty=(int) (tile/ntx);
  const int y=ty*WAVES+wave;
  const int x0=tx*SEG;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const T *taps=static_cast<const T *>(args.taps);
  const size_t pitch=(size_t) W*C;
  const bool row_ok=y < H;
  const Q *row=src+(size_t) (row_ok ? y : H-1)*pitch;

  // stage the strip: sample i is input column clamp(x0-shift+i)
  for (int i=lane; i < NS; i+=64)
    {
      int xx=x0-args.shift+i;
      xx=xx < 0 ? 0 : (xx > W-1 ? W-1 : xx);
      Q v[C];
      load_pixel<Q,C>(row+(size_t) xx*C,v);
      store_pixel<Q,C>(strip+(size_t) lds_slot<R>(i)*C,v);
    }
  __syncthreads();
  if (!row_ok)
    return;

  Acc acc;
  acc.init((T) args.bias);
  const int NJ=R+K-1;
  const int base=lane*(R+1);                  // lds_slot(lane*R)
  Q cur[C],nxt[C];
  load_pixel<Q,C>(strip+(size_t) base*C,cur);
  auto fetch_next=[&](int j)
  {
    int jn=j+1 < NJ ? j+1 : j;
    load_pixel<Q,C>(strip+(size_t) (base+jn+jn/R)*C,nxt);
  };
  auto rotate=[&]()
  {
#pragma unroll
    for (int c=0; c < C; c++)
      cur[c]=nxt[c];
  };
  int j=0;
  const int ramp=(R-1) < NJ ? (R-1) : NJ;
  for ( ; j < ramp; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        {
          int t=j-r;
          if ((t >= 0) && (t < K))
            acc.tap(r,taps[t],in);
        }
      rotate();
    }
  for ( ; j < K; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        acc.tap(r,taps[j-r],in);
      rotate();
    }
  for ( ; j < NJ; j++)
    {
      fetch_next(j);
      typename Acc::In in=Acc::prepare(cur);
#pragma unroll
      for (int r=0; r < R; r++)
        {
          int t=j-r;
          if ((t >= 0) && (t < K))
            acc.tap(r,taps[t],in);
        }
      rotate();
    }
  unsigned changed=0;
  const int xo=x0+lane*R;
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int x=xo+r;
      if (x < W)
        {
          Q center[C],out[C];
          int ci=lane*R+r+args.shift;         // strip index of input column x
          load_pixel<Q,C>(strip+(size_t) lds_slot<R>(ci)*C,center);
          changed+=acc.finish(r,center,args.copy_mask,out,(T) args.bias);
          store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}


// =================================================================== blocked
// Q16 kernels.  Same register blocking (each lane owns R consecutive outputs
// along the filter axis and streams the R+K-1 inputs they depend on once),
// but the input stream is cut into blocks of U samples and the tap table is
// zero-padded by R-1 entries on both sides: inside a block the tap that
// output r takes from sample jj is  table[jb + (jj-r+R-1)], a compile-time
// offset from the wave-uniform block base, so one block needs R+U-1 taps that
// are fetched with a few scalar loads into SGPRs and every FMA reads its tap
// from a fixed SGPR.  No per-sample tap reloads, no ramp-up/ramp-down branches
// (the zero taps make the edge samples contribute nothing; Q16 samples are
// always finite, so  s + 0*p == s  exactly and the EXACT order is unchanged).
// The samples of block b+1 are fetched into registers while block b is
// accumulated.  (Where the taps live: stage_taps, conv1d_pass.hpp.)
template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_column_blocked(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows;
  const unsigned ntx=(unsigned) ((W+63)/64);
  const unsigned nty=(unsigned) ((H+R*WAVES-1)/(R*WAVES));
  const unsigned total=ntx*nty;
  const unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  const unsigned tile=(id & 7u)*per+(id >> 3);       // XCD-aware: see conv_column_kernel
  if (tile >= total)
    return;
  const int tx=(int) (tile/nty),ty=(int) (tile%nty);
  const int x=tx*64+lane;
  const int xc=x < W ? x : W-1;
  const int y0=(ty*WAVES+wave)*R;
  const Q *src=static_cast<const Q *>(args.src)+(size_t) xc*C;
  Q *dst=static_cast<Q *>(args.dst);
  const size_t pitch=(size_t) W*C;
  const int ybase=y0-args.shift;
  const int nblocks=args.nblocks;
  const T *table=stage_taps<T,A::taps_in_lds>(args,smem_raw,nblocks*U+R-1,false);
  if (y0 >= H)
    return;

  Acc acc;
  acc.init((T) args.bias);
  Q nxt[U][C];
  // interior tiles (every row this wave touches exists) address row jb+jj as
  // uniform base + jj*pitch + lane offset: two scalar adds per row and an
  // SGPR-base load, instead of a clamp and a 64-bit multiply per row
  const bool interior=(ybase >= 0) && (ybase+nblocks*U <= H);
  const unsigned lane_off=(unsigned) xc*(unsigned) (C*sizeof(Q));
  const char *base0=reinterpret_cast<const char *>(args.src);
  const size_t pitch_bytes=pitch*sizeof(Q);
  auto fetch=[&](int jb)
  {
    if (interior)
      {
        const char *rowp=base0+(size_t) (ybase+jb)*pitch_bytes;
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            load_pixel<Q,C>(reinterpret_cast<const Q *>(rowp+lane_off),nxt[jj]);
            rowp+=pitch_bytes;
          }
      }
    else
      {
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            int yy=ybase+jb+jj;
            yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
            load_pixel<Q,C>(src+(size_t) yy*pitch,nxt[jj]);
          }
      }
  };
  fetch(0);
  for (int b=0; b < nblocks; b++)
    {
      const int jb=b*U;
      T tw[R+U-1];
#pragma unroll
      for (int i=0; i < R+U-1; i++)
        tw[i]=table[jb+i];
      Q cur[U][C];
#pragma unroll
      for (int jj=0; jj < U; jj++)
#pragma unroll
        for (int c=0; c < C; c++)
          cur[jj][c]=nxt[jj][c];
      if (b+1 < nblocks)
        fetch(jb+U);
#pragma unroll
      for (int jj=0; jj < U; jj++)
        {
          typename Acc::In in=Acc::prepare(cur[jj]);
#pragma unroll
          for (int r=0; r < R; r++)
            acc.tap(r,tw[jj-r+R-1],in);
        }
    }
  unsigned changed=0;
  // the centre pixel is only needed for the `changed` count and for Copy channels
  const bool need_center=(args.changed != nullptr) || (args.copy_mask != 0);
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int y=y0+r;
      if (y < H)
        {
          Q center[C],out[C];
#pragma unroll
          for (int c=0; c < C; c++)
            center[c]=(Q) 0;
          if (need_center)
            load_pixel<Q,C>(src+(size_t) y*pitch,center);
          unsigned ch=acc.finish(r,center,args.copy_mask,out,(T) args.bias,args.changed != nullptr);
          if (x < W)
            {
              if (args.unsharp_src != nullptr)
                unsharp_on_the_way_out<Q,C>(args,(size_t) y*W+(size_t) x,out);
              store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
              changed+=ch;
            }
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

// Row pass: a wave stages the 63R+NJ input pixels its 64R outputs depend on in
// LDS (coalesced global reads), with one padding slot every R samples so the
// stride-R reads of the 64 lanes fall on distinct banks; blocks are R samples
// long (U == R) so the slot of sample jb+jj is  base + jb + jb/R + jj.
template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_row_blocked(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  static_assert((R%U) == 0,"a block of U samples must not straddle an LDS padding slot");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows;
  const int nblocks=args.nblocks;
  const int SEG=64*R;                         // outputs per wave
  const int NS=63*R+nblocks*U;                // input samples per wave
  const int slots=NS+NS/R+1;
  const int table_bytes=A::taps_in_lds ? (((nblocks*U+R-1)*(int) sizeof(T)+15) & ~15) : 0;
  Q *strip=reinterpret_cast<Q *>(smem_raw+table_bytes)+(size_t) wave*slots*C;

  const unsigned ntx=(unsigned) ((W+SEG-1)/SEG);
  const unsigned nty=(unsigned) ((H+WAVES-1)/WAVES);
  const unsigned total=ntx*nty;
  const unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  const unsigned tile=(id & 7u)*per+(id >> 3);
  if (tile >= total)
    return;
  const int tx=(int) (tile%ntx),ty=(int) (tile/ntx);
  const int y=ty*WAVES+wave;
  const int x0=tx*SEG;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const T *table=stage_taps<T,A::taps_in_lds>(args,smem_raw,nblocks*U+R-1,true);
  const size_t pitch=(size_t) W*C;
  const bool row_ok=y < H;
  const Q *row=src+(size_t) (row_ok ? y : H-1)*pitch;

  // stage the strip in batches: all loads of a batch are in flight before the
  // first LDS store waits for one (a load-store loop would pay one memory
  // latency per 64 samples)
  {
    constexpr int BATCH=10;
    for (int i0=lane; i0 < NS; i0+=64*BATCH)
      {
        Q v[BATCH][C];
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int i=i0+64*k;
            int xx=x0-args.shift+(i < NS ? i : NS-1);
            xx=xx < 0 ? 0 : (xx > W-1 ? W-1 : xx);
            load_pixel<Q,C>(row+(size_t) xx*C,v[k]);
          }
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int i=i0+64*k;
            if (i < NS)
              store_pixel<Q,C>(strip+(size_t) (i+i/R)*C,v[k]);
          }
      }
  }
  __syncthreads();
  if (!row_ok)
    return;

  Acc acc;
  acc.init((T) args.bias);
  const Q *mine=strip+(size_t) lane*(R+1)*C;     // slot of sample lane*R
  // the samples of block b+1 are read from LDS into registers while block b is
  // accumulated (sample jb+jj sits in slot jb + jb/R + jj: U divides R)
  Q nxt[U][C];
  auto fetch=[&](int jb)
  {
    const Q *blk=mine+(size_t) (jb+jb/R)*C;
#pragma unroll
    for (int jj=0; jj < U; jj++)
      load_pixel<Q,C>(blk+(size_t) jj*C,nxt[jj]);
  };
  fetch(0);
  for (int b=0; b < nblocks; b++)
    {
      const int jb=b*U;
      T tw[R+U-1];
#pragma unroll
      for (int i=0; i < R+U-1; i++)
        tw[i]=table[jb+i];
      Q cur[U][C];
#pragma unroll
      for (int jj=0; jj < U; jj++)
#pragma unroll
        for (int c=0; c < C; c++)
          cur[jj][c]=nxt[jj][c];
      if (b+1 < nblocks)
        fetch(jb+U);
#pragma unroll
      for (int jj=0; jj < U; jj++)
        {
          typename Acc::In in=Acc::prepare(cur[jj]);
#pragma unroll
          for (int r=0; r < R; r++)
            acc.tap(r,tw[jj-r+R-1],in);
        }
    }
  unsigned changed=0;
  const int xo=x0+lane*R;
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int x=xo+r;
      if (x < W)
        {
          Q center[C],out[C];
          int ci=lane*R+r+args.shift;           // strip index of input column x
          load_pixel<Q,C>(strip+(size_t) (ci+ci/R)*C,center);
          changed+=acc.finish(r,center,args.copy_mask,out,(T) args.bias,args.changed != nullptr);
          store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

template<typename Q,int C,bool BLEND,class A,int R,int U>
static MhStatus launch_blocked(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  typedef typename A::T T;
  constexpr int WAVES=4;
  const int K=p.ntaps;
  const int nblocks=(R+K-1+U-1)/U;
  const int entries=blocked_table_entries<R,U>(nblocks);
  // padded, reversed tap table: entry e multiplies, for output r, the sample
  // j = e-(R-1)+r; U spare zero entries behind
  const std::vector<T> host=reversed_taps<T>(p,R-1,entries+U-(R-1)-K);
  Temp taps;
  MH_TRY(upload_table(taps,src.device,src.stream,host.data(),host.size()*sizeof(T)));
  Conv1DArgs args=conv1d_args(src,dst,p,roles,changed,taps.ptr);
  args.nblocks=nblocks;
  const int W=args.columns,H=args.rows;
  if (vertical)
    return launch_with_dynamic_lds("conv_column",&conv_column_blocked<Q,C,BLEND,A,R,U,WAVES>,
      xcd_grid(column_tiles<R,WAVES>(W,H)),64*WAVES,(size_t) tap_table_bytes<A>(entries),src.stream,args);
  const int slots=strip_slots<R>(blocked_strip_samples<R,U>(nblocks));
  return launch_with_dynamic_lds("conv_row",&conv_row_blocked<Q,C,BLEND,A,R,U,WAVES>,
    xcd_grid(row_tiles<R,WAVES>(W,H)),64*WAVES,row_pass_lds<Q,C,WAVES>(tap_table_bytes<A>(entries),slots),
    src.stream,args);
}


// ================================================================ triangular
// (the walk: tri_accumulate, conv1d_pass.hpp)
template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_column_tri(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows,K=args.ntaps;
  const unsigned ntx=(unsigned) ((W+63)/64);
  const unsigned nty=(unsigned) ((H+R*WAVES-1)/(R*WAVES));
  const unsigned total=ntx*nty;
  const unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  const unsigned tile=(id & 7u)*per+(id >> 3);       // XCD-aware: see conv_column_kernel
  if (tile >= total)
    return;
  const int tx=(int) (tile/nty),ty=(int) (tile%nty);
  const int x=tx*64+lane;
  const int xc=x < W ? x : W-1;
  const int y0=(ty*WAVES+wave)*R;
  const Q *src=static_cast<const Q *>(args.src)+(size_t) xc*C;
  Q *dst=static_cast<Q *>(args.dst);
  const size_t pitch=(size_t) W*C;
  const int ybase=y0-args.shift;
  const T *table=stage_taps<T,A::taps_in_lds>(args,smem_raw,K,false);
  if (y0 >= H)
    return;

  Acc acc;
  acc.init((T) args.bias,K);
  Q nxt[U][C];
  const bool interior=(ybase >= 0) && (ybase+R+K+U <= H);
  const char *base0=reinterpret_cast<const char *>(args.src)+(size_t) xc*(size_t) (C*sizeof(Q));
  const size_t pitch_bytes=pitch*sizeof(Q);
  auto fetch_u=[&](int pos)
  {
    if (interior)
      {
        const char *rowp=base0+(size_t) (ybase+pos)*pitch_bytes;
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            load_pixel<Q,C>(reinterpret_cast<const Q *>(rowp),nxt[jj]);
            rowp+=pitch_bytes;
          }
      }
    else
      {
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            int yy=ybase+pos+jj;
            yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
            load_pixel<Q,C>(src+(size_t) yy*pitch,nxt[jj]);
          }
      }
  };
  auto fetch_1=[&](int pos)
  {
    int yy=ybase+pos;
    yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
    load_pixel<Q,C>(src+(size_t) yy*pitch,nxt[0]);
  };
  tri_accumulate<Q,C,BLEND,A,R,U>(acc,table,K,fetch_u,fetch_1,nxt);

  unsigned changed=0;
  const bool need_center=(args.changed != nullptr) || (args.copy_mask != 0);
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int y=y0+r;
      if (y < H)
        {
          Q center[C],out[C];
#pragma unroll
          for (int c=0; c < C; c++)
            center[c]=(Q) 0;
          if (need_center)
            load_pixel<Q,C>(src+(size_t) y*pitch,center);
          unsigned ch=acc.finish(r,center,args.copy_mask,out,(T) args.bias,args.changed != nullptr,
            make_reference<Q,C,BLEND,A>(args,true,xc,y));
          if (x < W)
            {
              if (args.unsharp_src != nullptr)
                unsharp_on_the_way_out<Q,C>(args,(size_t) y*W+(size_t) x,out);
              store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
              changed+=ch;
            }
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}


// Column pass with the rows staged through LDS.  In conv_column_tri every wave
// fetches its own R+K-1 rows, so an image row is requested (R+K-1)/R = 5.9 times
// (R=16, K=79) and, with a 4 MB L2 per XCD, most of those re-reads go back to the
// fabric (PMC: 3.47 GB per launch against 1.07 GB algorithmic).  Here a workgroup
// of WAVES waves stages the WAVES*R+K-1 rows of its 64-column strip once, with
// batched coalesced loads, and the waves take their samples from LDS (lane = column
// => each row read is one conflict-free 512-byte ds_read_b64 sweep).
template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_column_lds(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows,K=args.ntaps;
  const int table_bytes=A::taps_in_lds ? ((K*(int) sizeof(T)+15) & ~15) : 0;
  Q *tile=reinterpret_cast<Q *>(smem_raw+table_bytes);
  const unsigned ntx=(unsigned) ((W+63)/64);
  const unsigned nty=(unsigned) ((H+R*WAVES-1)/(R*WAVES));
  const unsigned total=ntx*nty;
  const unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  const unsigned tile_id=(id & 7u)*per+(id >> 3);    // XCD-aware: see conv_column_kernel
  if (tile_id >= total)
    return;
  const int tx=(int) (tile_id/nty),ty=(int) (tile_id%nty);
  const int x=tx*64+lane;
  const int yb=ty*WAVES*R;                             // first output row of the workgroup
  const int y0=yb+wave*R;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const size_t pitch=(size_t) W*C;
  const T *table=stage_taps<T,A::taps_in_lds>(args,smem_raw,K,true);
  // stage rows yb-shift .. yb-shift+nrows-1 (edge clamp, cache.c:2663-2679), 64 pixels each
  const int nrows=WAVES*R+K-1;
  {
    constexpr int BATCH=18;
    const int items=nrows*64;
    const int x0=tx*64;
    for (int i0=(int) threadIdx.x; i0 < items; i0+=64*WAVES*BATCH)
      {
        Q v[BATCH][C];
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int idx=i0+64*WAVES*k;
            idx=idx < items ? idx : items-1;
            int yy=yb-args.shift+(idx >> 6),xx=x0+(idx & 63);
            yy=yy < 0 ? 0 : (yy > H-1 ? H-1 : yy);
            xx=xx > W-1 ? W-1 : xx;
            load_pixel<Q,C>(src+(size_t) yy*pitch+(size_t) xx*C,v[k]);
          }
#pragma unroll
        for (int k=0; k < BATCH; k++)
          if (i0+64*WAVES*k < items)
            store_pixel<Q,C>(tile+(size_t) (i0+64*WAVES*k)*C,v[k]);
      }
  }
  __syncthreads();
  if (y0 >= H)
    return;

  Acc acc;
  acc.init((T) args.bias,K);
  const Q *mine=tile+((size_t) wave*R*64+(size_t) lane)*C;      // sample j lives at mine + j*64*C
  Q nxt[U][C];
  auto fetch_u=[&](int pos)
  {
#pragma unroll
    for (int jj=0; jj < U; jj++)
      {
        int j=pos+jj;
        j=j < R+K-1 ? j : R+K-2;                                 // the last prefetch may run over
        load_pixel<Q,C>(mine+(size_t) j*64*C,nxt[jj]);
      }
  };
  auto fetch_1=[&](int pos)
  {
    load_pixel<Q,C>(mine+(size_t) pos*64*C,nxt[0]);
  };
  tri_accumulate<Q,C,BLEND,A,R,U>(acc,table,K,fetch_u,fetch_1,nxt);

  unsigned changed=0;
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int y=y0+r;
      if (y < H)
        {
          Q center[C],out[C];
          load_pixel<Q,C>(mine+(size_t) (r+args.shift)*64*C,center);   // input row y
          unsigned ch=acc.finish(r,center,args.copy_mask,out,(T) args.bias,args.changed != nullptr,
            make_reference<Q,C,BLEND,A>(args,true,x < W ? x : W-1,y));
          if (x < W)
            {
              if (args.unsharp_src != nullptr)
                unsharp_on_the_way_out<Q,C>(args,(size_t) y*W+(size_t) x,out);
              store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
              changed+=ch;
            }
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
__global__ __launch_bounds__(64*WAVES)
void conv_row_tri(Conv1DArgs args)
{
  if (pass_not_wanted(args))
    return;
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int W=args.columns,H=args.rows,K=args.ntaps;
  const int SEG=64*R;                         // outputs per wave
  const int NS=63*R+R+K-1+U;                  // input samples per wave (+U: the C prefetch may run over)
  const int slots=NS+NS/R+1;
  const int table_bytes=A::taps_in_lds ? ((K*(int) sizeof(T)+15) & ~15) : 0;
  Q *strip=reinterpret_cast<Q *>(smem_raw+table_bytes)+(size_t) wave*slots*C;

  const unsigned ntx=(unsigned) ((W+SEG-1)/SEG);
  const unsigned nty=(unsigned) ((H+WAVES-1)/WAVES);
  const unsigned total=ntx*nty;
  const unsigned id=blockIdx.x;
  const unsigned per=(total+7u)/8u;
  const unsigned tile=(id & 7u)*per+(id >> 3);
  if (tile >= total)
    return;
  const int tx=(int) (tile%ntx),ty=(int) (tile/ntx);
  const int y=ty*WAVES+wave;
  const int x0=tx*SEG;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const T *table=stage_taps<T,A::taps_in_lds>(args,smem_raw,K,true);
  const size_t pitch=(size_t) W*C;
  const bool row_ok=y < H;
  const Q *row=src+(size_t) (row_ok ? y : H-1)*pitch;
  {
    constexpr int BATCH=10;
    for (int i0=lane; i0 < NS; i0+=64*BATCH)
      {
        Q v[BATCH][C];
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int i=i0+64*k;
            int xx=x0-args.shift+(i < NS ? i : NS-1);
            xx=xx < 0 ? 0 : (xx > W-1 ? W-1 : xx);
            load_pixel<Q,C>(row+(size_t) xx*C,v[k]);
          }
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int i=i0+64*k;
            if (i < NS)
              store_pixel<Q,C>(strip+(size_t) (i+i/R)*C,v[k]);
          }
      }
  }
  __syncthreads();
  if (!row_ok)
    return;

  Acc acc;
  acc.init((T) args.bias,K);
  const Q *mine=strip+(size_t) lane*(R+1)*C;     // slot of sample lane*R
  Q nxt[U][C];
  auto fetch_u=[&](int pos)
  {
    // U consecutive samples; a block may straddle a padding slot only when pos is not a
    // multiple of U inside R, which the single-sample phase makes possible: index each one
#pragma unroll
    for (int jj=0; jj < U; jj++)
      {
        const int j=pos+jj;
        load_pixel<Q,C>(mine+(size_t) (j+j/R)*C,nxt[jj]);
      }
  };
  auto fetch_1=[&](int pos)
  {
    load_pixel<Q,C>(mine+(size_t) (pos+pos/R)*C,nxt[0]);
  };
  tri_accumulate<Q,C,BLEND,A,R,U>(acc,table,K,fetch_u,fetch_1,nxt);

  unsigned changed=0;
  const int xo=x0+lane*R;
  // 16-byte pixels (float RGBA: the HDRI blur): a lane's R consecutive results are 64 scattered
  // 16-byte pieces per store instruction when the lane stores them itself.  They leave through the
  // wave's strip instead — dead once no centre sample is needed — as contiguous kilobytes (see
  // separable_row_sums_kernel).  Whole segments only; rows' last segments keep the direct stores.
  if constexpr (C*sizeof(Q) == 16)
    {
      constexpr int LS=R*16+16;                 // a lane's deposit + a 16-byte gap (banks)
      const bool whole=x0+SEG <= W;
      if (whole && (args.changed == nullptr) && (args.copy_mask == 0) && (64*LS <= slots*16))
        {
          unsigned char *stash=reinterpret_cast<unsigned char *>(strip);
#pragma unroll
          for (int r=0; r < R; r++)
            {
              Q center[C],out[C];
#pragma unroll
              for (int c=0; c < C; c++)
                center[c]=(Q) 0;
              (void) acc.finish(r,center,0u,out,(T) args.bias,false,make_reference<Q,C,BLEND,A>(args,false,xo+r,y));
              store_pixel<Q,C>(reinterpret_cast<Q *>(stash+lane*LS+r*16),out);
            }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE,"wavefront");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE,"wavefront");
          unsigned char *to=reinterpret_cast<unsigned char *>(dst+(size_t) y*pitch+(size_t) x0*C);
#pragma unroll
          for (int k=0; k < R; k++)
            {
              const int item=lane+64*k;           // 64 R pixels of 16 bytes
              const int from=item/R,within=item-from*R;
              const uint4 v=*reinterpret_cast<const uint4 *>(stash+from*LS+within*16);
              *reinterpret_cast<uint4 *>(to+(size_t) item*16)=v;
            }
          return;
        }
    }
  // a lane's R outputs are contiguous in the row: store them two pixels (16 bytes for
  // RGBA Q16) at a time — half the store instructions of this lane-strided pattern
  constexpr bool kPair=((R & 1) == 0) && (C*sizeof(Q) == 8);
#pragma unroll
  for (int r=0; r < R; r+=(kPair ? 2 : 1))
    {
      int x=xo+r;
      if (x < W)
        {
          Q center[C],out[C];
          int ci=lane*R+r+args.shift;           // strip index of input column x
          load_pixel<Q,C>(strip+(size_t) (ci+ci/R)*C,center);
          changed+=acc.finish(r,center,args.copy_mask,out,(T) args.bias,args.changed != nullptr,
            make_reference<Q,C,BLEND,A>(args,false,x,y));
          if constexpr (kPair)
            {
              if (x+1 < W)
                {
                  Q center1[C],out1[C];
                  int c1=ci+1;
                  load_pixel<Q,C>(strip+(size_t) (c1+c1/R)*C,center1);
                  changed+=acc.finish(r+1,center1,args.copy_mask,out1,(T) args.bias,args.changed != nullptr,
                    make_reference<Q,C,BLEND,A>(args,false,x+1,y));
                  Q both[2*C];
#pragma unroll
                  for (int c=0; c < C; c++)
                    {
                      both[c]=out[c];
                      both[C+c]=out1[c];
                    }
                  store_pixel<Q,2*C>(dst+(size_t) y*pitch+(size_t) x*C,both);
                  continue;
                }
            }
          store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,out);
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

// conv_column_lds's staged strip must fit twice per CU
constexpr size_t kColumnStagingLimit=80u*1024u;

template<typename Q,int C,bool BLEND,class A,int R,int U,int WAVES>
static MhStatus launch_tri_waves(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  typedef typename A::T T;
  const int K=p.ntaps;
  const std::vector<T> host=reversed_taps<T>(p);
  Temp taps;
  MH_TRY(upload_table(taps,src.device,src.stream,host.data(),host.size()*sizeof(T)));
  Conv1DArgs args=conv1d_args(src,dst,p,roles,changed,taps.ptr);
  const int W=args.columns,H=args.rows;
  if (vertical)
    {
      args.unsharp_src=p.unsharp_source;
      args.unsharp_gain=p.unsharp_gain;
      args.unsharp_threshold=p.unsharp_threshold;
      const unsigned grid=xcd_grid(column_tiles<R,WAVES>(W,H));
      // rows staged once per workgroup through LDS when the strip fits twice per CU
      const size_t lds_tile=column_lds_bytes<Q,C,A,R,WAVES>(K);
      if (lds_tile <= kColumnStagingLimit)
        return launch_with_dynamic_lds("conv_column",&conv_column_lds<Q,C,BLEND,A,R,U,WAVES>,grid,64*WAVES,
          lds_tile,src.stream,args);
      return launch_with_dynamic_lds("conv_column",&conv_column_tri<Q,C,BLEND,A,R,U,WAVES>,grid,64*WAVES,
        (size_t) tap_table_bytes<A>(K),src.stream,args);
    }
  const int slots=strip_slots<R>(tri_strip_samples<R,U>(K));
  return launch_with_dynamic_lds("conv_row",&conv_row_tri<Q,C,BLEND,A,R,U,WAVES>,
    xcd_grid(row_tiles<R,WAVES>(W,H)),64*WAVES,row_pass_lds<Q,C,WAVES>(tap_table_bytes<A>(K),slots),
    src.stream,args);
}

template<typename Q,int C,bool BLEND,class A,int R,int U>
static MhStatus launch_tri(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  typedef typename A::T T;
  // fp64 column pass: eight waves share a staged strip when it still fits twice per CU (142
  // rows for 79 taps: 73 KB): the K-1 halo rows are staged per 64 output rows instead of per 32
  // and every SIMD holds four waves instead of two — conv_column 1.43 -> 1.21 ms on 8192^2
  // (Tie64).  The f32 policy measured slower with 8 and 16 waves and stays at four.
  if ((sizeof(T) == 8) && vertical && (column_lds_bytes<Q,C,A,R,8>(p.ntaps) <= kColumnStagingLimit))
    return launch_tri_waves<Q,C,BLEND,A,R,U,8>(src,dst,vertical,p,roles,changed);
  return launch_tri_waves<Q,C,BLEND,A,R,U,4>(src,dst,vertical,p,roles,changed);
}

// ---------------------------------------------------------------- launcher
template<typename Q,int C,bool BLEND,class A,int R>
static MhStatus launch_one(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  typedef typename A::T T;
  constexpr int WAVES=4;
  const std::vector<T> host=reversed_taps<T>(p);
  Temp taps;
  MH_TRY(upload_table(taps,src.device,src.stream,host.data(),host.size()*sizeof(T)));
  const Conv1DArgs args=conv1d_args(src,dst,p,roles,changed,taps.ptr);
  const int W=args.columns,H=args.rows;
  if (vertical)
    return launch_with_dynamic_lds("conv_column",&conv_column_kernel<Q,C,BLEND,A,R,WAVES>,
      xcd_grid(column_tiles<R,WAVES>(W,H)),64*WAVES,0,src.stream,args);
  const int slots=strip_slots<R>(plain_strip_samples<R>(p.ntaps));
  return launch_with_dynamic_lds("conv_row",&conv_row_kernel<Q,C,BLEND,A,R,WAVES>,
    xcd_grid(row_tiles<R,WAVES>(W,H)),64*WAVES,row_pass_lds<Q,C,WAVES>(0,slots),src.stream,args);
}

// The frame's channel count and blend flag as template arguments of one of the three families:
// f(Layout<Q,C,BLEND>{}).
template<typename Q,class F>
static MhStatus for_layout(const View &src,const Roles &roles,F &&f)
{
  if ((src.channels < 1) || (src.channels > 4))
    return fail(MH_UNSUPPORTED,"%d channels",src.channels);
  return dispatch_channels_blend<Q>(src.channels,roles.blend && (roles.alpha == src.channels-1),f);
}

template<typename Q,class A,int R>
static MhStatus dispatch_plain(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  return for_layout<Q>(src,roles,[&](auto L) {
    return launch_one<Q,L.C,L.BLEND,A,R>(src,dst,vertical,p,roles,changed); });
}

template<class A,int R,int U>
static MhStatus dispatch_blocked(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  return for_layout<uint16_t>(src,roles,[&](auto L) {
    return launch_blocked<uint16_t,L.C,L.BLEND,A,R,U>(src,dst,vertical,p,roles,changed); });
}

template<class A,int R,int U,typename Q=uint16_t>
static MhStatus dispatch_tri(const View &src,const View &dst,bool vertical,
  const Conv1DParams &p,const Roles &roles,unsigned long long *changed)
{
  return for_layout<Q>(src,roles,[&](auto L) {
    return launch_tri<Q,L.C,L.BLEND,A,R,U>(src,dst,vertical,p,roles,changed); });
}

// FAST row pass of an alpha-weighted layout on the f32 vector kernels: the Quantum-rounded alpha
// it writes becomes a WEIGHT in a following column pass (BlurImage), where one level more or
// less in a small alpha moves the colour by many levels.  This audit recomputes every alpha
// result below kSmallAlpha (+1) levels as the reference does — fp64, its operation order
// (morphology.c:2941-2951), ClampToQuantum — so the intermediate alpha is bit-identical to the
// reference's wherever a level matters (the matrix-core kernels do the same inside their
// epilogue, mfma_common.hpp).  Frames without small alpha only pay one read of the alpha
// samples.
template<int C>
__global__ __launch_bounds__(256)
void conv_row_alpha_audit_kernel(const uint16_t *src,uint16_t *dst,int columns,int rows,
  const double *taps64,int K,int shift)
{
  const size_t total=(size_t) columns*(size_t) rows;
  for (size_t at=(size_t) blockIdx.x*256u+threadIdx.x; at < total; at+=(size_t) gridDim.x*256u)
    {
      if (dst[at*C+(C-1)] > 8192u)
        continue;
      const size_t y=at/(size_t) columns;
      const int x=(int) (at-y*(size_t) columns);
      const uint16_t *line=src+y*(size_t) columns*C;
      double sum=0.0;
      for (int v=0; v < K; v++)
        {
          int xx=x-shift+v;
          xx=xx < 0 ? 0 : (xx > columns-1 ? columns-1 : xx);
          sum=sum+taps64[v]*(double) line[(size_t) xx*C+(C-1)];
        }
      dst[at*C+(C-1)]=QuantumOps<uint16_t>::clamp(sum);
    }
}

static MhStatus launch_row_alpha_audit(const View &src,const View &dst,const Conv1DParams &params)
{
  const int K=params.ntaps;
  const std::vector<double> host=reversed_taps<double>(params);
  Temp taps;
  MH_TRY(upload_table(taps,src.device,src.stream,host.data(),host.size()*sizeof(double)));
  const size_t total=src.columns*src.rows;
  const unsigned blocks=(unsigned) ((total+255)/256 < 8192 ? (total+255)/256 : 8192);
  ProfileScope prof("conv_row_alpha_audit",src.stream);
  if (src.channels == 4)
    hipLaunchKernelGGL((conv_row_alpha_audit_kernel<4>),dim3(blocks),dim3(256),0,src.stream,
      static_cast<const uint16_t *>(src.pixels),static_cast<uint16_t *>(dst.pixels),(int) src.columns,
      (int) src.rows,taps.as<double>(),K,K-1-params.origin);
  else
    hipLaunchKernelGGL((conv_row_alpha_audit_kernel<2>),dim3(blocks),dim3(256),0,src.stream,
      static_cast<const uint16_t *>(src.pixels),static_cast<uint16_t *>(dst.pixels),(int) src.columns,
      (int) src.rows,taps.as<double>(),K,K-1-params.origin);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// What the launchers' choices of a policy ask about a kernel's taps (a tap that is not >= 0, a NaN
// included, counts as negative)
struct TapFacts
{
  bool all_non_negative;
  double sum,sum_of_magnitudes;
};

static TapFacts tap_facts(const Conv1DParams &params)
{
  TapFacts facts={true,0.0,0.0};
  for (int v=0; v < params.ntaps; v++)
    {
      facts.all_non_negative=facts.all_non_negative && (params.taps[v] >= 0.0);
      facts.sum+=params.taps[v];
      facts.sum_of_magnitudes+=std::fabs(params.taps[v]);
    }
  return facts;
}

// float Quantum under the tie check of Accum::finish(): its error bound holds for normalised positive taps
static bool normalised_positive(const TapFacts &facts)
{
  return facts.all_non_negative && (facts.sum <= 1.0+1.0e-9);
}

MhStatus launch_conv1d_column_unsharp(const View &rows,const View &dst,const View &original,
  const Conv1DParams &params,const Roles &roles,MhPrecision prec,double gain,double threshold,
  bool *handled)
{
  *handled=false;
  const bool is_float=rows.quantum != MH_QUANTUM_U16;
  if ((!is_float && (prec != MH_PRECISION_EXACT)) || (params.ntaps < 16) || (params.bias != 0.0) ||
      (original.columns != rows.columns) || (original.rows != rows.rows) ||
      (original.channels != rows.channels) || (original.quantum != rows.quantum) ||
      (option("MAGICKHIP_NO_FUSED_UNSHARP") != nullptr))
    return MH_OK;
  const TapFacts facts=tap_facts(params);
  if (!facts.all_non_negative || (is_float && !normalised_positive(facts)))
    return MH_OK;
  Conv1DParams with=params;
  with.unsharp_source=original.pixels;
  with.unsharp_gain=gain;
  with.unsharp_threshold=65535.0*threshold;    // QuantumRange*threshold, effect.c:4300
  *handled=true;
  if (is_float)
    return dispatch_tri<Tie64,8,8,float>(rows,dst,true,with,roles,nullptr);
  return dispatch_tri<Tie64,8,8>(rows,dst,true,with,roles,nullptr);
}

// One 1-D pass over [rows][columns][4] DOUBLES (un-normalised sums in, sums out): fused
// multiply-adds, nothing rounded to a Quantum — the passes of convolve_separable.hip.  The Views'
// `pixels` point at doubles; their quantum field is not looked at.
MhStatus launch_conv1d_sums64(const View &src,const View &dst,bool vertical,const Conv1DParams &params)
{
  Roles plain;
  plain.update_mask=0xfu;
  if (params.ntaps >= 16)
    return launch_tri<double,4,false,Fma64,8,8>(src,dst,vertical,params,plain,nullptr);
  return launch_one<double,4,false,Fma64,8>(src,dst,vertical,params,plain,nullptr);
}

MhStatus launch_conv1d_sums(const View &src,const View &dst,bool vertical,const Conv1DParams &params,
  bool blend,bool *handled)
{
  *handled=false;
  if ((params.ntaps < 2) || (params.origin < 0) || (params.origin >= params.ntaps) ||
      (option("MAGICKHIP_NO_MFMA") != nullptr))
    return MH_OK;
  const int K=params.ntaps;
  const std::vector<float> host=reversed_taps<float>(params);
  Temp taps;
  MH_TRY(upload_table(taps,src.device,src.stream,host.data(),host.size()*sizeof(float)));
  return launch_conv1d_mfma(src,dst,vertical,taps.as<float>(),K,K-1-params.origin,blend,
    vertical ? MFMA_FROM_SUMS : MFMA_TO_SUMS,handled);
}

MhStatus launch_conv1d_unsharp(const View &rows,const View &dst,const View &original,
  const Conv1DParams &params,bool blend,double gain,double threshold,bool *handled)
{
  *handled=false;
  if ((params.ntaps < 2) || (params.origin < 0) || (params.origin >= params.ntaps) ||
      (params.bias != 0.0) || (option("MAGICKHIP_NO_MFMA") != nullptr) ||
      (option("MAGICKHIP_NO_FUSED_UNSHARP") != nullptr))
    return MH_OK;
  const int K=params.ntaps;
  if (blend && !f16_taps_resolved(params.taps,K))
    return MH_OK;                                // (see launch_conv1d)
  const std::vector<float> host=reversed_taps<float>(params);
  Temp taps;
  MH_TRY(upload_table(taps,rows.device,rows.stream,host.data(),host.size()*sizeof(float)));
  return launch_conv1d_mfma(rows,dst,true,taps.as<float>(),K,K-1-params.origin,blend,MFMA_UNSHARP,
    handled,&original,gain,threshold,nullptr,f16_tap_scale(params.taps,K));
}

MhStatus launch_conv1d(const View &src,const View &dst,bool vertical,
  const Conv1DParams &params,const Roles &roles,MhPrecision prec,
  unsigned long long *changed)
{
  if ((src.columns != dst.columns) || (src.rows != dst.rows) ||
      (src.channels != dst.channels) || (src.quantum != dst.quantum))
    return fail(MH_BAD_ARGUMENT,"conv1d: source/destination geometry mismatch");
  if (roles.blend && (roles.alpha != src.channels-1))
    return fail(MH_UNSUPPORTED,"alpha channel must be the last channel");
  if ((params.ntaps < 1) || (params.origin < 0) || (params.origin >= params.ntaps))
    return fail(MH_BAD_ARGUMENT,"conv1d: bad kernel geometry");
  const TapFacts facts=tap_facts(params);
  // Alpha-weighted channels with taps of both signs: sum(k*alpha) can come out near zero, where
  // the reference's PerceptibleReciprocal clamp decides the pixel and no reduced-precision sum
  // stays within a level of it.  FAST keeps to the fp64 kernels there.
  if ((prec == MH_PRECISION_FAST) && roles.blend && !facts.all_non_negative)
    prec=MH_PRECISION_EXACT;
  // ... and taps of both signs with a large gain on any layout: the float sums are good to 2^-21 of
  // sum|k|*65535, which cancellation does not shrink
  if ((prec == MH_PRECISION_FAST) && !facts.all_non_negative && !(facts.sum_of_magnitudes <= 8.0))
    prec=MH_PRECISION_EXACT;
  // ... and alpha-weighted channels under a kernel whose outer taps are tiny beside the rest (BlurImage
  // with a radius far beyond its sigma): where such a tap is the only one that meets an opaque sample — a
  // sprite on a transparent ground — it IS the result (sum(k*alpha*p)/sum(k*alpha), morphology.c:2968-2977),
  // and neither the f16 terms nor the f32 sums resolve it.  The fp64 kernels take those.
  if ((prec == MH_PRECISION_FAST) && roles.blend && !f16_taps_resolved(params.taps,params.ntaps))
    prec=MH_PRECISION_EXACT;
  if (src.quantum == MH_QUANTUM_U16)
    {
      if (prec == MH_PRECISION_FAST)
        {
          // RGBA with alpha-weighted colour channels (BlurImage's case), or 3/4 independent
          // channels (RGB, CMYK): the banded-matrix formulation on the f16 matrix cores,
          // convolve_mfma.hip
          if ((roles.blend ? (src.channels == 4) && (roles.alpha == 3) :
               (src.channels == 3) || (src.channels == 4)) && (roles.copy_mask == 0) &&
              (params.bias == 0.0) && (changed == nullptr) && (option("MAGICKHIP_NO_MFMA") == nullptr))
            {
              const int K=params.ntaps;
              // one table: K doubles (the exact recomputation of ambiguous small alpha levels),
              // then K floats; both in the reversed walk of morphology.c:2746
              std::vector<double> host=reversed_taps<double>(params,0,(K+1)/2);
              float *host_floats=reinterpret_cast<float *>(host.data()+K);
              for (int v=0; v < K; v++)
                host_floats[v]=(float) host[(size_t) v];
              const void *taps=nullptr;
              std::shared_ptr<void> keep;       // until the launch below is enqueued
              MH_TRY(shared_table(src.device,src.stream,host.data(),host.size()*sizeof(double),&taps,&keep));
              const double *taps64=static_cast<const double *>(taps);
              bool handled=false;
              MH_TRY(launch_conv1d_mfma(src,dst,vertical,reinterpret_cast<const float *>(taps64+K),K,
                K-1-params.origin,roles.blend,MFMA_Q16,&handled,nullptr,0.0,0.0,taps64,
                f16_tap_scale(params.taps,K)));
              if (handled)
                return MH_OK;
            }
          // long kernels: the triangular kernels with 32 outputs per lane; short ones: blocked
          // K >= R+1: the ramp-free triangular kernels (measured +7.5 % at K=79 on MI355X;
          // R=24/32 variants were slower: 240 VGPRs leave two waves per SIMD)
          if (params.ntaps >= 24)
            MH_TRY((dispatch_tri<Fast32,16,4>(src,dst,vertical,params,roles,changed)));
          else
            MH_TRY((dispatch_blocked<Fast32,16,4>(src,dst,vertical,params,roles,changed)));
          // alpha-weighted layouts (gray + alpha, RGBA): small alpha results exact, see above
          if (!vertical && roles.blend && (params.bias == 0.0) && ((roles.copy_mask >> roles.alpha) & 1u) == 0 &&
              ((src.channels == 2) || (src.channels == 4)))
            MH_TRY(launch_row_alpha_audit(src,dst,params));
          return MH_OK;
        }
      if (params.ntaps >= 16)
        {
          // fused sums + reference-order recomputation of the results they cannot decide: the
          // same bits at less than half the fp64 work (device_common.hpp, Tie64).  Positive taps
          // only (a weighted sum of both signs can cancel: the error bound is relative to the
          // sum of magnitudes, not to the result), no bias, no change count.
          if (facts.all_non_negative && (params.bias == 0.0) && (changed == nullptr))
            return dispatch_tri<Tie64,8,8>(src,dst,vertical,params,roles,changed);
          return dispatch_tri<Exact64,8,8>(src,dst,vertical,params,roles,changed);
        }
      return dispatch_blocked<Exact64,8,8>(src,dst,vertical,params,roles,changed);
    }
  // float Quantum always accumulates in double: an FP32 sum cannot stay
  // within 1 ULP of a float result.  Long normalised positive kernels (BlurImage's) take the
  // fused sums with the float-rounding tie check of Accum::finish(): the same bits as the
  // reference's order at 4 fused multiply-adds per tap instead of 11 separately rounded operations.
  if ((params.ntaps >= 16) && (params.bias == 0.0) && (changed == nullptr) && normalised_positive(facts))
    {
      // (the row pass with four samples in flight instead of eight: 138 registers instead of 194,
      // three waves a SIMD — the fp64 pipe sustains more with more waves, tools/ubench/
      // fma_f64_rate.hip — 1.25 -> 1.15 ms per 8192^2 frame; the column pass keeps its 182
      // registers either way and is slower with four)
      if (!vertical)
        return dispatch_tri<Tie64,8,4,float>(src,dst,vertical,params,roles,changed);
      return dispatch_tri<Tie64,8,8,float>(src,dst,vertical,params,roles,changed);
    }
  return dispatch_plain<float,Exact64,8>(src,dst,vertical,params,roles,changed);
}

} // namespace mh
