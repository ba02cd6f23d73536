// The accumulators of the 1-D convolve passes (convolve.hip, convolve_folded.hip): what a lane keeps for its R
// outputs, how a sample enters them under each arithmetic policy (device_common.hpp), and how a sum becomes a
// Quantum — with the reference's own operation order for the results a fused sum cannot decide.
#pragma once
#include "device_common.hpp"

namespace mh {

// (conv1d_reference_sample: device_common.hpp)

// finish()'s fallback for policies without a tie check
struct NoReference
{
  __device__ __forceinline__ unsigned operator()(int) const { return 0u; }
};

// ... and the real one: output (x,y) of a pass over `src`
template<typename Q,int C,bool BLEND>
struct ReferenceSample
{
  const Q *src;
  const double *taps;
  int W,H,K,shift,x,y;
  bool vertical;
  double bias;
  __device__ __forceinline__ Q operator()(int c) const
  {
    return conv1d_reference_sample<Q,C,BLEND>(src,W,H,vertical,x,y,c,taps,K,shift,bias);
  }
};

// ---------------------------------------------------------------- Accum
template<typename Q,int C,bool BLEND,class A,int R>
struct Accum
{
  typedef typename A::T T;
  // channel pairs live in 2-element vectors so the f32 policy can issue one
  // v_pk_fma_f32 per pair: a wave can issue only one VALU instruction per ~4.6
  // cycles (tools/ubench), so the packed form halves the issue slots a wave needs
  // and a single ready wave keeps the SIMD's FMA pipe busy.
  typedef T V2 __attribute__((ext_vector_type(2)));
  static constexpr int NP=(C+1)/2;
  V2 sv[R][NP];
  T g[R];
  // float Quantum under the tie check: the largest |sample| each channel has streamed (the error bound of a
  // sum is relative to it) and (2K+6)*2^-53, see finish().  Kept as a float, two samples an instruction
  // (v_max3_f32 with |x| source modifiers) where a running fp64 maximum of the premultiplied samples cost one
  // v_max_f64 a sample and channel.  (The OR of the samples' bit patterns — one v_or3_b32 for two — is a bound too,
  // but not a tight one: exponents 0x7f and 0x80 OR to 0xff, so a frame holding a 1.5 beside a 2.5 has an infinite
  // "bound" and every lane takes the reference's order: the row pass of a uniform-random frame ran 3.5x slower,
  // profiles/r6_notes/float_passes_and_dilate_order.txt.)  A NaN is dropped by the maximum as it was by
  // v_max_f64 (the sums are NaN then, and decide nothing); an Inf makes the bound infinite.
  static constexpr bool kTracksMagnitude=A::tie_check && (sizeof(Q) == 4);
  float seen[kTracksMagnitude ? C : 1];
  T error_unit;
#define MH_S(r,c) sv[r][(c) >> 1][(c) & 1]

  struct In { V2 pv[NP]; T a; };
#define MH_P(in,c) (in).pv[(c) >> 1][(c) & 1]

  // the sum of output r's channel c, for the passes that store sums instead of Quantum samples
  __device__ __forceinline__ T sum(int r,int c) const { return MH_S(r,c); }

  __device__ __forceinline__ void init(T bias,int ntaps=0)
  {
#pragma unroll
    for (int r=0; r < R; r++)
      {
#pragma unroll
        for (int c=0; c < C; c++)
          MH_S(r,c)=A::premultiply ? (T) 0 : bias;
        g[r]=(T) 0;
      }
    error_unit=(T) 0;
    if constexpr (kTracksMagnitude)
      {
#pragma unroll
        for (int c=0; c < C; c++)
          seen[c]=0.0f;
        error_unit=(T) (2*ntaps+6)*(T) 1.1102230246251565e-16;
      }
  }

  __device__ __forceinline__ void observe(const Q (&q)[C])
  {
    if constexpr (kTracksMagnitude)
      {
#pragma unroll
        for (int c=0; c < C; c++)
          asm("v_max_f32 %0, %1, |%2|" : "=v"(seen[c]) : "v"(seen[c]),"v"(q[c]));
      }
  }

  __device__ __forceinline__ void observe(const Q (&q0)[C],const Q (&q1)[C])
  {
    if constexpr (kTracksMagnitude)
      {
#pragma unroll
        for (int c=0; c < C; c++)
          asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(seen[c]) : "v"(seen[c]),"v"(q0[c]),"v"(q1[c]));
      }
  }

  // ... as a magnitude of what channel c's sums are made of: alpha * p for a weighted colour channel
  // (max |alpha * p| <= max |alpha| * max |p|; the product of two floats is exact in fp64)
  __device__ __forceinline__ T magnitude(int c) const
  {
    if constexpr (kTracksMagnitude)
      {
        T m=(T) seen[c];
        if (BLEND && A::premultiply && (c != C-1))
          m=m*(T) seen[C-1];
        return m;
      }
    else
      return (T) 0;
  }

  static __device__ __forceinline__ In prepare(const Q (&q)[C])
  {
    In in;
#pragma unroll
    for (int q2=0; q2 < NP; q2++)
      in.pv[q2]=V2{(T) 0,(T) 0};
#pragma unroll
    for (int c=0; c < C; c++)
      MH_P(in,c)=(T) q[c];
    in.a=(T) 0;
    if constexpr (BLEND)
      {
        if constexpr (A::premultiply)
          {
            // gamma*pixel = (sum k*QS*alpha*p)/(sum k*QS*alpha): QuantumScale cancels, so
            // the FAST policy weights by the raw alpha quantum
            // whole channel pairs with one packed multiply, the odd colour channel alone
            const T alpha=MH_P(in,C-1);
#pragma unroll
            for (int q2=0; q2 < (C-1)/2; q2++)
              in.pv[q2]=in.pv[q2]*V2{alpha,alpha};
            if constexpr (((C-1) & 1) != 0)
              MH_P(in,C-2)=A::mul(alpha,MH_P(in,C-2));
          }
        else
          in.a=A::mul((T) kQS,MH_P(in,C-1));    // alpha=QuantumScale*GetPixelAlpha(): morphology.c:2766, :2965
      }
    return in;
  }

  __device__ __forceinline__ void packed_mac(int r,T kv,const In &in)
  {
    V2 k2={kv,kv};
#pragma unroll
    for (int q=0; q < C/2; q++)
      sv[r][q]=__builtin_elementwise_fma(k2,in.pv[q],sv[r][q]);
    if constexpr ((C & 1) != 0)
      MH_S(r,C-1)=A::mac(MH_S(r,C-1),kv,MH_P(in,C-1));
  }

  __device__ __forceinline__ void tap(int r,T kv,const In &in)
  {
    if constexpr (BLEND)
      {
        if constexpr (A::premultiply)
          {
            packed_mac(r,kv,in);
            // gamma = sum kv*QuantumScale*alpha = QuantumScale*(s[alpha]-bias): no
            // separate accumulator in this mode (finish() derives it)
          }
        else
          {
            // pixel+=alpha*(*k)*pixels[i]; gamma+=alpha*(*k);  morphology.c:2767-2768
            T w=A::mul(in.a,kv);
#pragma unroll
            for (int c=0; c < C-1; c++)
              MH_S(r,c)=A::add(MH_S(r,c),A::mul(w,MH_P(in,c)));
            g[r]=A::add(g[r],w);
            MH_S(r,C-1)=A::mac(MH_S(r,C-1),kv,MH_P(in,C-1));      // alpha channel: no weighting
          }
      }
    else
      {
        if constexpr (A::premultiply)
          packed_mac(r,kv,in);
        else
          {
#pragma unroll
            for (int c=0; c < C; c++)
              MH_S(r,c)=A::mac(MH_S(r,c),kv,MH_P(in,c));          // morphology.c:2750
          }
      }
  }

  // returns the number of channels that count as "changed" (morphology.c:2772, :3199)
  // reference(c): the sample recomputed in the reference's order (Tie64's doubtful results)
  template<class Reference=NoReference>
  __device__ __forceinline__ unsigned finish(int r,const Q (&center)[C],uint32_t copy_mask,
    Q (&out)[C],T bias,bool count_changed=true,const Reference &reference=Reference()) const
  {
    unsigned changed=0;
    if constexpr (A::tie_check)
      {
        // fused fp64 sums of alpha-premultiplied samples (bias 0, no change count: the launcher
        // sends everything else to Exact64).  S_c = sum k*alpha*p, S_a = sum k*alpha.
        static_assert(((sizeof(Q) == 2) || (sizeof(Q) == 4)) && (sizeof(T) == 8),
          "the tie check is for Q16 or float samples summed in fp64");
        if constexpr (sizeof(Q) == 4)
          {
            // float Quantum (HDRI): the result is the fp64 value rounded to float, so a "tie" is a
            // value closer to the midpoint of two neighbouring floats than the two summation
            // orders can differ.  Per channel that is at most (2K+6)*2^-53 * max|sample| * sum|k|
            // (K roundings of each order's running sum plus the reference's three per term; the
            // launcher admits normalised positive taps only, sum|k| <= 1); the alpha-weighted
            // colour channels add the quotient's share.  NaN fails every comparison below and
            // lands in the reference path, as do infinities, denormals and powers of two (whose
            // lower neighbour is half as far away).
            T inverse=(T) 1,alpha_error=(T) 0;
            bool doubtful=false;
            if constexpr (BLEND)
              {
                const T sa=MH_S(r,C-1);
                doubtful=(sa != (T) 0) && !(__builtin_fabs((T) kQS*sa) >= (T) kEps*(T) 1.000001);
                inverse=sa == (T) 0 ? (T) 0 : perceptible_reciprocal_fast(sa);
                alpha_error=error_unit*magnitude(C-1);
              }
#pragma unroll
            for (int c=0; c < C; c++)
              {
                if ((copy_mask >> c) & 1u)
                  {
                    out[c]=center[c];
                    continue;
                  }
                T value=MH_S(r,c);
                T error=error_unit*magnitude(c);
                if (BLEND && (c != C-1))
                  {
                    value=value*inverse;
                    error=__builtin_fma(__builtin_fabs(value),alpha_error,error)*__builtin_fabs(inverse)+
                      __builtin_fabs(value)*(T) 1.0e-15;
                  }
                const float nearest=(float) value;
                const uint32_t bits=__float_as_uint(nearest);
                const int exponent=(int) ((bits >> 23) & 0xffu);
                const bool power_of_two=(bits & 0x7fffffu) == 0u;
                const bool ordinary=(exponent != 0xff) && ((exponent != 0) || ((bits & 0x7fffffffu) == 0u));
                // half an ulp of `nearest`: 2^(e-127-24), a quarter below a power of two
                const int half_exponent=(exponent > 0 ? exponent : 1)-151-(power_of_two ? 1 : 0);
                const T half_ulp=__longlong_as_double((long long) (half_exponent+1023) << 52);
                const T distance=__builtin_fabs(value-(T) nearest);
                const bool decided=ordinary && (half_ulp-distance > error);
                Q level=nearest;
                if (!decided || (doubtful && BLEND && (c != C-1)))
                  level=reference(c);
                out[c]=level;
              }
            return 0;
          }
        T inverse=(T) 1;
        bool doubtful=false;
        if constexpr (BLEND)
          {
            const T sa=MH_S(r,C-1);
            // PerceptibleReciprocal acts below MagickEpsilon (the reference's gamma is QuantumScale*S_a)
            doubtful=(sa != (T) 0) && !((T) kQS*sa >= (T) kEps);
            inverse=sa == (T) 0 ? (T) 0 : perceptible_reciprocal_fast(sa);
          }
#pragma unroll
        for (int c=0; c < C; c++)
          {
            if ((copy_mask >> c) & 1u)
              {
                out[c]=center[c];
                continue;
              }
            T value=MH_S(r,c);
            if (BLEND && (c != C-1))
              value=value*inverse;
            const T shifted=value+(T) 0.5;
            const T fraction=shifted-__builtin_floor(shifted);
            const bool tie=(fraction < (T) kTieMargin) || (fraction > (T) 1-(T) kTieMargin);
            Q level=QuantumOps<Q>::clamp(value);
            if (tie || (doubtful && BLEND && (c != C-1)))
              level=(Q) reference(c);
            out[c]=level;
          }
        return 0;
      }
    else if constexpr (A::premultiply)
      {
        // FAST epilogue, all in f32 and branch-free.  s[] holds the un-biased sums
        // S_c = sum k*alpha*p (colour), S_a = sum k*alpha; the reference's
        // gamma*pixel is (bias*QuantumRange + S_c)/S_a, the alpha channel bias + S_a.
        // v_rcp_f32(0) = inf and 0*inf = NaN convert to 0, which is what
        // PerceptibleReciprocal's clamp yields for an all-transparent window.
        static_assert(sizeof(Q) == 2,"the FAST policy is Q16 only");
        T inv=(T) 1,cbias=bias;
        if constexpr (BLEND)
          {
            inv=__builtin_amdgcn_rcpf(MH_S(r,C-1));
            cbias=bias*(T) kQR;
          }
#pragma unroll
        for (int c=0; c < C; c++)
          {
            T pixel=MH_S(r,c);
            if (BLEND && (c != C-1))
              pixel=(pixel+cbias)*inv;
            else
              pixel=pixel+bias;
            if (count_changed)
              {
                // compares the un-normalised sum (morphology.c:2772, :3199)
                T raw=BLEND && (c != C-1) ? (T) kQS*MH_S(r,c)+bias : MH_S(r,c)+bias;
                T d=raw-(T) center[c];
                if (!((copy_mask >> c) & 1u) && ((d < (T) 0 ? -d : d) >= (T) kEps))
                  changed++;
              }
            // ClampToQuantum (quantum.h:86-97): v_cvt_u32_f32 maps NaN and negatives to 0
            unsigned q=(unsigned) (pixel+(T) 0.5);
            q=q > 65535u ? 65535u : q;
            out[c]=((copy_mask >> c) & 1u) ? center[c] : (Q) q;
          }
        return changed;
      }
    T gsum=g[r];
#pragma unroll
    for (int c=0; c < C; c++)
      {
        if ((copy_mask >> c) & 1u)
          {
            out[c]=center[c];
            continue;
          }
        double pixel=(double) MH_S(r,c);
        if (fabs(pixel-(double) center[c]) >= kEps)
          changed++;
        if (BLEND && (c != C-1))
          pixel=perceptible_reciprocal((double) gsum)*pixel;
        out[c]=QuantumOps<Q>::clamp(pixel);
      }
    return changed;
  }
#undef MH_S
#undef MH_P
};

} // namespace mh
