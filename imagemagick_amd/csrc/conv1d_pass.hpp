// What the 1-D convolve passes of convolve.hip and convolve_folded.hip share: the kernel arguments, the
// unsharp epilogue, the tap table on the device, the triangular walk, and on the host side the launch geometry
// (one function per quantity), the reversed tap table, the argument fill and the launch.
#pragma once
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "conv1d_accum.hpp"
#include <vector>

namespace mh {

struct Conv1DArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int ntaps;
  int shift;                 // K-1-origin: offset of the first input sample
  double bias;
  uint32_t copy_mask;
  const void *taps;          // T[K], reversed so that taps[v] multiplies input o-shift+v
  unsigned long long *changed;
  int nblocks;               // blocked kernels: number of U-sample blocks of the padded tap table
  int wave_bytes;            // separable_row_sums_kernel: bytes of LDS a wave owns (strip / stash)
  // triangular column kernels: UnsharpMaskImage's epilogue on the way out (effect.c:4364-4369);
  // unsharp_src = the unblurred frame, or NULL
  const void *unsharp_src;
  double unsharp_gain,unsharp_threshold;
  const unsigned *only_if;   // nullptr, or: every workgroup leaves at once unless the word is set:
  unsigned only_if_token;    //   0: set = not zero;  otherwise: set = equal to the token (no clearing launch needed)
};

// ------------------------------------------------------------------ geometry
// What every launcher sizes its grid and its dynamic LDS with, one function per quantity.  The kernels still
// spell the same quantities (NS, slots, table_bytes, nrows, ntx, nty) in their own bodies, and an edit to one
// side must be made on the other: routing a kernel's NS through one of these functions, nothing else changed,
// moved conv_row_blocked<uint16_t,1,false,Fast32,16,4,4> from 47 to 53 VGPRs under this compiler, and the
// kernels' register counts are pinned.

struct TileGrid
{
  unsigned ntx,nty;
  __host__ __device__ __forceinline__ unsigned count() const { return ntx*nty; }
};

// column pass: a workgroup of WAVES waves owns 64 columns x WAVES*R rows
template<int R,int WAVES> __host__ __device__ __forceinline__ TileGrid column_tiles(int W,int H)
{
  return TileGrid{(unsigned) ((W+63)/64),(unsigned) ((H+R*WAVES-1)/(R*WAVES))};
}

// row pass: a wave owns 64*R outputs of one row, a workgroup WAVES rows
template<int R,int WAVES> __host__ __device__ __forceinline__ TileGrid row_tiles(int W,int H)
{
  constexpr int SEG=64*R;
  return TileGrid{(unsigned) ((W+SEG-1)/SEG),(unsigned) ((H+WAVES-1)/WAVES)};
}

// workgroups to launch: the tiles, rounded up to whole rounds of the eight XCDs (the kernels' XCD-aware tile order)
static inline unsigned xcd_grid(TileGrid tiles)
{
  return ((tiles.count()+7u)/8u)*8u;
}

// input samples a wave of a row pass stages for its 64*R outputs: the plain pass; the blocked pass (the last
// lane's stream is nblocks blocks of U); the triangular pass (+U: the C prefetch may run over)
template<int R> __host__ __device__ __forceinline__ int plain_strip_samples(int K) { return 64*R+K-1; }
template<int R,int U> __host__ __device__ __forceinline__ int blocked_strip_samples(int nblocks) { return 63*R+nblocks*U; }
template<int R,int U> __host__ __device__ __forceinline__ int tri_strip_samples(int K) { return 63*R+R+K-1+U; }

// LDS slot of strip sample i: one padding slot every R samples, so the lanes of
// a wave (stride R samples) hit distinct banks ...
template<int R> __host__ __device__ __forceinline__ int lds_slot(int i) { return i+i/R; }
// ... and the slots a strip of NS samples takes
template<int R> __host__ __device__ __forceinline__ int strip_slots(int NS) { return NS+NS/R+1; }

// entries of the blocked kernels' tap table: zero-padded by R-1 in front, to whole blocks behind
template<int R,int U> __host__ __device__ __forceinline__ int blocked_table_entries(int nblocks) { return nblocks*U+R-1; }

// bytes in front of the strips that a policy's tap table of `entries` takes in LDS, 16-byte rounded (the column
// passes with nothing behind the table ask for the rounded size as well: the same allocation granule)
template<class A> __host__ __device__ __forceinline__ int tap_table_bytes(int entries)
{
  return A::taps_in_lds ? ((entries*(int) sizeof(typename A::T)+15) & ~15) : 0;
}

// a row pass's dynamic LDS: the table, then one strip of `slots` pixels per wave
template<typename Q,int C,int WAVES> static inline size_t row_pass_lds(int table_bytes,int slots)
{
  return (size_t) table_bytes+(size_t) WAVES*slots*C*sizeof(Q);
}

// conv_column_lds: the rows a workgroup stages, 64 pixels each, behind the table
template<int R,int WAVES> __host__ __device__ __forceinline__ int column_lds_rows(int K) { return WAVES*R+K-1; }
template<typename Q,int C,class A,int R,int WAVES> static inline size_t column_lds_bytes(int K)
{
  return (size_t) tap_table_bytes<A>(K)+(size_t) column_lds_rows<R,WAVES>(K)*64*C*sizeof(Q);
}

static __device__ __forceinline__ bool pass_not_wanted(const Conv1DArgs &args)
{
  if (args.only_if == nullptr)
    return false;
  const unsigned word=*args.only_if;
  return args.only_if_token == 0u ? word == 0u : word != args.only_if_token;
}

// ------------------------------------------------------------------ column epilogue
// blurred sample -> unsharp-masked sample, as unsharp_kernel (pointwise.hip) does in its own pass
template<typename Q,int C>
static __device__ __forceinline__ void unsharp_on_the_way_out(const Conv1DArgs &args,size_t pixel,Q (&out)[C])
{
  Q p[C];
  load_pixel<Q,C>(static_cast<const Q *>(args.unsharp_src)+pixel*C,p);
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((args.copy_mask >> c) & 1u)
        {
          out[c]=p[c];
          continue;
        }
      double value=(double) p[c]-(double) out[c];
      if (fabs(2.0*value) < args.unsharp_threshold)
        value=(double) p[c];
      else
        value=(double) p[c]+args.unsharp_gain*value;
      out[c]=QuantumOps<Q>::clamp(value);
    }
}

template<typename Q,int C,bool BLEND,class A>
static __device__ __forceinline__ auto make_reference(const Conv1DArgs &args,bool vertical,int x,int y)
{
  if constexpr (A::tie_check)
    return ReferenceSample<Q,C,BLEND>{static_cast<const Q *>(args.src),static_cast<const double *>(args.taps),
      args.columns,args.rows,args.ntaps,args.shift,x,y,vertical,args.bias};
  else
    return NoReference();
}

// ------------------------------------------------------------------ tap table on the device
// Where the taps live matters on gfx950 (tools/ubench/valu_rate.hip, 4 waves/SIMD):
// v_fmac_f32 with an SGPR multiplier sustains 64.6 TFLOP/s, the all-VGPR form
// 122 TFLOP/s.  The f32 policy therefore stages the tap table in LDS once per
// workgroup and reads each block's R+U-1 taps with broadcast ds_reads into
// VGPRs; the f64 policy (no such penalty measured) keeps scalar loads.
template<typename T,bool IN_LDS>
static __device__ __forceinline__ const T *stage_taps(const Conv1DArgs &args,unsigned char *smem,
  int count,bool sync_done)
{
  const T *global=static_cast<const T *>(args.taps);
  if constexpr (!IN_LDS)
    return global;
  else
    {
      T *lds=reinterpret_cast<T *>(smem);
      for (int i=(int) threadIdx.x; i < count; i+=(int) blockDim.x)
        lds[i]=global[i];
      if (!sync_done)
        __syncthreads();
      return lds;
    }
}

// ================================================================ triangular
// The blocked kernels spend (R-1)/(R+K-1) of their multiply-adds on the
// zero-padded ramp taps (15 % at K=79, R=16).  This walk splits the sample
// stream of a lane's R outputs into
//   A  samples 0 .. R-1           output r takes sample j only when r <= j
//   B  samples R .. K-2           every output takes every sample (blocks of U, then single samples)
//   C  samples K-1 .. K+R-2       output r takes sample K-1+s only when r >= s
// A and C are fully unrolled with compile-time (sample, output) pairs, so exactly
// K*R*C multiply-adds are issued and larger R (fewer, longer sample streams per
// output) becomes profitable.  Tap table: the reversed taps t[0..K-1], t[v]
// multiplying sample j for output r when v = j-r.  Requires K >= R+1.
template<typename Q,int C,bool BLEND,class A,int R,int U,class FETCHU,class FETCH1>
static __device__ __forceinline__ void tri_accumulate(Accum<Q,C,BLEND,A,R> &acc,
  const typename A::T *table,int K,FETCHU fetch_u,FETCH1 fetch_1,Q (&nxt)[U][C])
{
  typedef typename A::T T;
  typedef Accum<Q,C,BLEND,A,R> Acc;
  static_assert((R%U) == 0,"R must be a multiple of U");
  static_assert((U%2) == 0,"samples are observed two at a time");
  const int M=K-1-R;                       // samples of phase B
  const int nfull=M/U,nrem=M-nfull*U;
  const int b2_begin=R+nfull*U,b2_end=K-1;
  auto prefetch=[&](int pos)
  {
    if ((pos >= b2_begin) && (pos < b2_end))
      fetch_1(pos);
    else
      fetch_u(pos);
  };
  Q cur[U][C];
  auto grab=[&]()
  {
#pragma unroll
    for (int jj=0; jj < U; jj++)
#pragma unroll
      for (int c=0; c < C; c++)
        cur[jj][c]=nxt[jj][c];
  };
  int pos=0;
  fetch_u(0);
  // ---- A
  {
    T ta[R];
#pragma unroll
    for (int i=0; i < R; i++)
      ta[i]=table[i];
#pragma unroll
    for (int c0=0; c0 < R/U; c0++)
      {
        grab();
        prefetch(pos+U);
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            typename Acc::In in=Acc::prepare(cur[jj]);
            if ((jj & 1) == 0)
              acc.observe(cur[jj],cur[jj+1]);
#pragma unroll
            for (int r=0; r < R; r++)
              if (r <= c0*U+jj)
                acc.tap(r,ta[c0*U+jj-r],in);
          }
        pos+=U;
      }
  }
  // ---- B, blocks of U samples
  for (int b=0; b < nfull; b++)
    {
      grab();
      prefetch(pos+U);
      T tw[R+U-1];
#pragma unroll
      for (int i=0; i < R+U-1; i++)
        tw[i]=table[pos-(R-1)+i];
#pragma unroll
      for (int jj=0; jj < U; jj++)
        {
          typename Acc::In in=Acc::prepare(cur[jj]);
          if ((jj & 1) == 0)
            acc.observe(cur[jj],cur[jj+1]);
#pragma unroll
          for (int r=0; r < R; r++)
            acc.tap(r,tw[jj-r+R-1],in);
        }
      pos+=U;
    }
  // ---- B, the M mod U remaining samples one at a time
  for (int b=0; b < nrem; b++)
    {
      grab();
      prefetch(pos+1);
      T tw[R];
#pragma unroll
      for (int i=0; i < R; i++)
        tw[i]=table[pos-(R-1)+i];
      typename Acc::In in=Acc::prepare(cur[0]);
      acc.observe(cur[0]);
#pragma unroll
      for (int r=0; r < R; r++)
        acc.tap(r,tw[R-1-r],in);
      pos+=1;
    }
  // ---- C
  {
    T tc[R];
#pragma unroll
    for (int i=0; i < R; i++)
      tc[i]=table[K-R+i];
#pragma unroll
    for (int c0=0; c0 < R/U; c0++)
      {
        grab();
        if (c0+1 < R/U)
          fetch_u(pos+U);
#pragma unroll
        for (int jj=0; jj < U; jj++)
          {
            typename Acc::In in=Acc::prepare(cur[jj]);
            if ((jj & 1) == 0)
              acc.observe(cur[jj],cur[jj+1]);
#pragma unroll
            for (int r=0; r < R; r++)
              if (r >= c0*U+jj)
                acc.tap(r,tc[R-1+c0*U+jj-r],in);
          }
        pos+=U;
      }
  }
}

// ------------------------------------------------------------------ host side
// The tap table a pass uploads: taps reversed, host[lead+v] = values[K-1-v] (k starts at the last value and
// walks backwards, morphology.c:2746 / :2919), between `lead` and `tail` zero entries.
template<typename T>
static std::vector<T> reversed_taps(const Conv1DParams &p,int lead=0,int tail=0)
{
  const int K=p.ntaps;
  std::vector<T> host((size_t) (lead+K+tail),(T) 0);
  for (int v=0; v < K; v++)
    host[(size_t) (lead+v)]=(T) p.taps[K-1-v];
  return host;
}

// no unsharp epilogue, nblocks and wave_bytes 0: the launchers that have those set them
static inline Conv1DArgs conv1d_args(const View &src,const View &dst,const Conv1DParams &p,const Roles &roles,
  unsigned long long *changed,const void *taps)
{
  Conv1DArgs args;
  args.unsharp_src=nullptr;
  args.unsharp_gain=0.0;
  args.unsharp_threshold=0.0;
  args.src=src.pixels;
  args.dst=dst.pixels;
  args.columns=(int) src.columns;
  args.rows=(int) src.rows;
  args.ntaps=p.ntaps;
  args.shift=p.ntaps-1-p.origin;     // offset.x / offset.y, morphology.c:2623-2624
  args.bias=p.bias;
  args.copy_mask=roles.copy_mask;
  args.taps=taps;
  args.changed=changed;
  args.nblocks=0;
  args.wave_bytes=0;
  args.only_if=p.only_if;
  args.only_if_token=p.only_if_token;
  return args;
}

// One pass under its profile label (launch_dynamic_lds, layout_dispatch.hpp); more than the CU's 160 KB is refused.
template<class... MORE>
static MhStatus launch_with_dynamic_lds(const char *label,void (*kernel)(Conv1DArgs,MORE...),unsigned grid,
  unsigned block,size_t lds,hipStream_t stream,const Conv1DArgs &args,MORE... more)
{
  if (lds > 160u*1024u)
    return fail(MH_UNSUPPORTED,"row kernel of %d taps needs %zu bytes of LDS",args.ntaps,lds);
  ProfileScope prof(label,stream);
  return launch_dynamic_lds(kernel,dim3(grid),dim3(block),lds,stream,args,more...);
}

} // namespace mh
