// Device colour maths that more than one translation unit uses: the fp64 XYZ / Lab conversions and the
// HSB / HSL round trips (colorspace.hip, pointwise.hip), and the f32 pieces of the FAST sRGB -> Lab route
// (colorspace.hip, histogram.hip).  Restated from MagickCore/colorspace-private.h and colorspace.c; the line of
// each formula is cited at its restatement.
#pragma once

#include "device_common.hpp"
#include "pixel_intensity.hpp"

namespace mh {

// D65, colorspace-private.h:25-44
#define MH_ILL_X 0.95047
#define MH_ILL_Y 1.00000
#define MH_ILL_Z 1.08883
#define MH_CIE_EPSILON (216.0/24389.0)
#define MH_CIE_K (24389.0/27.0)

// ConvertRGBToXYZ, colorspace-private.h:759-779
static __device__ void rgb_to_xyz(double red,double green,double blue,double &X,double &Y,double &Z)
{
  double r=kQS*decode_pixel_gamma(red);
  double g=kQS*decode_pixel_gamma(green);
  double b=kQS*decode_pixel_gamma(blue);
  X=(0.4123955889674142161*r)+(0.3575834307637148171*g)+(0.1804926473817015735*b);
  Y=(0.2125862307855955516*r)+(0.7151703037034108499*g)+(0.07220049864333622685*b);
  Z=(0.01929721549174694484*r)+(0.1191838645808485318*g)+(0.9504971251315797660*b);
}

// ConvertXYZToRGB, colorspace-private.h:72-94
static __device__ void xyz_to_rgb(double X,double Y,double Z,double &red,double &green,double &blue)
{
  double r=(3.240969941904521*X)+(-1.537383177570093*Y)+(-0.498610760293*Z);
  double g=(-0.96924363628087*X)+(1.87596750150772*Y)+(0.041555057407175*Z);
  double b=(0.055630079696993*X)+(-0.20397695888897*Y)+(1.056971514242878*Z);
  double gb=g < b ? g : b;
  double mn=r < gb ? r : gb;
  if (mn < 0.0)
    {
      r-=mn;
      g-=mn;
      b-=mn;
    }
  red=encode_pixel_gamma(kQR*r);
  green=encode_pixel_gamma(kQR*g);
  blue=encode_pixel_gamma(kQR*b);
}

// pow(t,1.0/3.0) for t in (CIEEpsilon, ~1.2].  The device's generic fp64 pow costs
// ~150 instructions; this is a float cbrt seed refined by two Newton steps whose
// residual t-y^3 is formed exactly (product split with an FMA) and whose 1/(3y^2)
// only needs float accuracy.  Error < 1 ulp of the true cube root; libm's
// pow(t,1.0/3.0) (exponent 1/3-1.85e-17) lies within 0.6 ulp of it as well, so the
// two agree to ~2 double ulps: identical after rounding to Q16, within the 1 float
// ULP the Lab tests allow for float Quantum.
static __device__ __forceinline__ double cube_root(double t)
{
  // seed: 2^(log2(t)/3) on the transcendental unit (~1e-6 relative), not libm's cbrtf
  const float seed=__builtin_amdgcn_exp2f(__builtin_amdgcn_logf((float) t)*0.333333343f);
  double y=(double) seed;
  const double inv=(double) __builtin_amdgcn_rcpf(3.0f*seed*seed);
#pragma unroll
  for (int it=0; it < 2; it++)
    {
      double yy=y*y;
      double yy_lo=__builtin_fma(y,y,-yy);            // y*y = yy + yy_lo exactly
      double res=__builtin_fma(-yy,y,t);               // t - yy*y (one rounding)
      res=__builtin_fma(-yy_lo,y,res);
      y=__builtin_fma(res,inv,y);
    }
  return y;
}

// x/d for a compile-time constant d without the division sequence: q=RN(x*RN(1/d)) refined
// twice with exact FMA residuals.  After the first refinement q is a faithful quotient, and
// a faithful quotient corrected once more by r*RN(1/d) is the correctly rounded one
// (Markstein's theorem; needs a significand of d that is not all ones — true of every
// constant used here), i.e. the same double the reference's `/` produces.  Non-finite
// quotients pass through unrefined (inf-inf would turn them into NaN).
static __device__ __forceinline__ double div_const(double x,const double d,const double y)
{
  double q=x*y;
  double r=__builtin_fma(-d,q,x);
  double q1=__builtin_fma(r,y,q);
  r=__builtin_fma(-d,q1,x);
  q1=__builtin_fma(r,y,q1);
  return __builtin_isfinite(q) ? q1 : q;
}
#define MH_DIV(x,d) div_const((x),(d),1.0/(d))

// ConvertXYZToLab, colorspace-private.h:1066-1089
static __device__ void xyz_to_lab(double X,double Y,double Z,double &L,double &a,double &b)
{
  double x,y,z;
  const double xr=MH_DIV(X,MH_ILL_X),yr=Y,zr=MH_DIV(Z,MH_ILL_Z);     // Y/1.0 is Y
  if (xr > MH_CIE_EPSILON)
    x=cube_root(xr);
  else
    x=MH_DIV(MH_DIV(MH_CIE_K*X,MH_ILL_X)+16.0,116.0);
  if (yr > MH_CIE_EPSILON)
    y=cube_root(yr);
  else
    y=MH_DIV(MH_CIE_K*Y+16.0,116.0);
  if (zr > MH_CIE_EPSILON)
    z=cube_root(zr);
  else
    z=MH_DIV(MH_DIV(MH_CIE_K*Z,MH_ILL_Z)+16.0,116.0);
  L=MH_DIV((116.0*y)-16.0,100.0);
  a=MH_DIV(500.0*(x-y),255.0)+0.5;
  b=MH_DIV(200.0*(y-z),255.0)+0.5;
}

// ConvertLabToXYZ, colorspace-private.h:531-557
static __device__ void lab_to_xyz(double L,double a,double b,double &X,double &Y,double &Z)
{
  double y=MH_DIV(L+16.0,116.0);
  double x=y+MH_DIV(a,500.0);
  double z=y-MH_DIV(b,200.0);
  if ((x*x*x) > MH_CIE_EPSILON)
    x=(x*x*x);
  else
    x=MH_DIV(116.0*x-16.0,MH_CIE_K);
  if (L > (MH_CIE_K*MH_CIE_EPSILON))
    y=(y*y*y);
  else
    y=MH_DIV(L,MH_CIE_K);
  if ((z*z*z) > MH_CIE_EPSILON)
    z=(z*z*z);
  else
    z=MH_DIV(116.0*z-16.0,MH_CIE_K);
  X=MH_ILL_X*x;
  Y=MH_ILL_Y*y;
  Z=MH_ILL_Z*z;
}

// FAST sRGB -> Lab on RGBA Q16 (config C4): the same expressions in f32 with the hardware
// log2 / exp2 for the 2.4 power and the cube roots.  Error budget in Quantum levels: the decode is
// good to 1e-6 relative, the cube roots to 3e-7, so L (x 65535 * 1.16) is within 0.03 and a, b
// (x 65535 * 500/255 of a difference of two roots) within 0.1 of the fp64 value: the rounded
// level differs from the reference's by at most one (MH_PRECISION_FAST's contract).  ~80 VALU
// slots per pixel against ~400 fp64-rate slots of the table kernel: the kernel becomes a stream.
static __device__ __forceinline__ float srgb_decode_fast(float x)
{
  // DecodePixelGamma, pixel.c:318-324, on [0,1]
  const float curve=__builtin_amdgcn_exp2f(2.4f*__builtin_amdgcn_logf((x+0.055f)*(1.0f/1.055f)));
  return x <= 0.0404482362771076f ? x*(1.0f/12.92f) : curve;
}

static __device__ __forceinline__ float lab_f_fast(float t)
{
  // ConvertXYZToLab, colorspace-private.h:1066-1089: cube root above epsilon, linear below.  Both sides are
  // computed and one is selected: as a branch, the dark lanes of a wave — there almost always are some — made the
  // wave run both sides behind six exec-mask switches per pixel pair.  (log2 of a t <= 0 is NaN / -inf: not selected.)
  float root=__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(t)*(1.0f/3.0f));
  asm volatile("" : "+v"(root));               // (evaluated here, for every lane: not sunk behind the comparison)
  const float line=__builtin_fmaf((float) (MH_CIE_K/116.0),t,(float) (16.0/116.0));
  return t > (float) MH_CIE_EPSILON ? root : line;
}

// The decode as a table in LDS: 2048 linear pieces of the curve, (value, rise) per piece.  The
// curve's second derivative is at most 3.1, so a piece is within (1/2048)^2/8*3.1 = 9e-8 of it —
// a tenth of the hardware log2/exp2 route's error — for a conversion, a multiply, a fraction, one
// ds_read_b64 and one FMA per sample instead of two quarter-rate transcendentals and six other
// operations.  Both FAST kernels decode through it (the one-call Lab + ContrastStretch leaves the
// frame TransformImageColorspace leaves, bit for bit).
constexpr int kDecodePieces=2048;
static __device__ __forceinline__ void build_decode_table(float2 *table)
{
  for (int i=(int) threadIdx.x; i < kDecodePieces; i+=(int) blockDim.x)
    {
      const float here=srgb_decode_fast((float) i*(1.0f/kDecodePieces));
      const float next=srgb_decode_fast((float) (i+1)*(1.0f/kDecodePieces));
      table[i]=make_float2(here,next-here);
    }
}

static __device__ __forceinline__ float srgb_decode_table(const float2 *table,unsigned quantum)
{
  // quantum/65535 in pieces; 65535 is the END of the last piece (fraction 1)
  const float at=(float) quantum*((float) kDecodePieces/65535.0f);
  const float whole=__builtin_fminf(__builtin_floorf(at),(float) (kDecodePieces-1));
  const float2 piece=table[(int) whole];
  return __builtin_fmaf(at-whole,piece.y,piece.x);
}

static __device__ __forceinline__ uint2 srgb_to_lab_fast_pixel(uint2 px,const float2 *decode)
{
  const float r=srgb_decode_table(decode,px.x & 0xffffu);
  const float g=srgb_decode_table(decode,px.x >> 16);
  const float b=srgb_decode_table(decode,px.y & 0xffffu);
  // (fused multiply-adds written out: the library is compiled with -ffp-contract=off for the EXACT kernels' sake,
  // and this f32 form has its own error budget; the illuminants folded into the X and Z rows)
  constexpr float ix=(float) (1.0/MH_ILL_X),iz=(float) (1.0/MH_ILL_Z);
  const float X=__builtin_fmaf(0.4123955889674142161f*ix,r,__builtin_fmaf(0.3575834307637148171f*ix,g,(0.1804926473817015735f*ix)*b));
  const float Y=__builtin_fmaf(0.2125862307855955516f,r,__builtin_fmaf(0.7151703037034108499f,g,0.07220049864333622685f*b));
  const float Z=__builtin_fmaf(0.01929721549174694484f*iz,r,__builtin_fmaf(0.1191838645808485318f*iz,g,(0.9504971251315797660f*iz)*b));
  const float fx=lab_f_fast(X),fy=lab_f_fast(Y),fz=lab_f_fast(Z);
  const float L=__builtin_fmaf(1.16f,fy,-0.16f);
  const float a=__builtin_fmaf(500.0f/255.0f,fx-fy,0.5f);
  const float bb=__builtin_fmaf(200.0f/255.0f,fy-fz,0.5f);
  // ClampToQuantum: v_cvt_pknorm_u16 clamps to [0,1] and rounds to nearest
  typedef unsigned short pk2 __attribute__((ext_vector_type(2)));
  const pk2 la=__builtin_amdgcn_cvt_pknorm_u16(L,a);
  const pk2 b0=__builtin_amdgcn_cvt_pknorm_u16(bb,0.0f);
  return make_uint2((unsigned) la[0] | ((unsigned) la[1] << 16),(unsigned) b0[0] | (px.y & 0xffff0000u));
}

// HSB and HSL round trips in fp64 exactly as the CPU path writes them (every expression in
// the reference's order; -ffp-contract=off): ConvertRGBToHSB / ConvertHSBToRGB
// colorspace-private.h:867-908 / :292-365, ConvertRGBToHSL / ConvertHSLToRGB
// colorspace.c:597-640 / :307-378.
static __device__ void rgb_to_hsb(double red,double green,double blue,double &hue,double &saturation,
  double &brightness)
{
  hue=0.0;
  saturation=0.0;
  brightness=0.0;
  double mn=red < green ? red : green;
  if (blue < mn)
    mn=blue;
  double mx=red > green ? red : green;
  if (blue > mx)
    mx=blue;
  if (fabs(mx) < kEps)
    return;
  const double delta=mx-mn;
  saturation=delta/mx;
  brightness=kQS*mx;
  if (fabs(delta) < kEps)
    return;
  if (fabs(red-mx) < kEps)
    hue=(green-blue)/delta;
  else if (fabs(green-mx) < kEps)
    hue=2.0+(blue-red)/delta;
  else
    hue=4.0+(red-green)/delta;
  hue/=6.0;
  if (hue < 0.0)
    hue+=1.0;
}

static __device__ void hsb_to_rgb(double hue,double saturation,double brightness,double &red,
  double &green,double &blue)
{
  if (fabs(saturation) < kEps)
    {
      red=kQR*brightness;
      green=red;
      blue=red;
      return;
    }
  const double h=6.0*(hue-floor(hue));
  const double f=h-floor(h);
  const double p=brightness*(1.0-saturation);
  const double q=brightness*(1.0-saturation*f);
  const double t=brightness*(1.0-(saturation*(1.0-f)));
  switch ((int) h)
  {
    case 1: red=kQR*q; green=kQR*brightness; blue=kQR*p; break;
    case 2: red=kQR*p; green=kQR*brightness; blue=kQR*t; break;
    case 3: red=kQR*p; green=kQR*q; blue=kQR*brightness; break;
    case 4: red=kQR*t; green=kQR*p; blue=kQR*brightness; break;
    case 5: red=kQR*brightness; green=kQR*p; blue=kQR*q; break;
    default: red=kQR*brightness; green=kQR*t; blue=kQR*p; break;        // 0
  }
}

static __device__ void rgb_to_hsl(double red,double green,double blue,double &hue,double &saturation,
  double &lightness)
{
  const double r=kQS*red,g=kQS*green,b=kQS*blue;
  const double gb_max=g > b ? g : b,gb_min=g < b ? g : b;
  const double mx=r > gb_max ? r : gb_max,mn=r < gb_min ? r : gb_min;
  const double c=mx-mn;
  lightness=(mx+mn)/2.0;
  if (c <= 0.0)
    {
      hue=0.0;
      saturation=0.0;
      return;
    }
  if (fabs(mx-r) < kEps)
    {
      hue=(g-b)/c;
      if (g < b)
        hue+=6.0;
    }
  else if (fabs(mx-g) < kEps)
    hue=2.0+(b-r)/c;
  else
    hue=4.0+(r-g)/c;
  hue*=60.0/360.0;
  if (lightness <= 0.5)
    saturation=c*perceptible_reciprocal(2.0*lightness);
  else
    saturation=c*perceptible_reciprocal(2.0-2.0*lightness);
}

static __device__ void hsl_to_rgb(double hue,double saturation,double lightness,double &red,
  double &green,double &blue)
{
  double h=hue*360.0,c;
  if (lightness <= 0.5)
    c=2.0*lightness*saturation;
  else
    c=(2.0-2.0*lightness)*saturation;
  const double mn=lightness-0.5*c;
  h-=360.0*floor(h/360.0);
  h/=60.0;
  const double x=c*(1.0-fabs(h-2.0*floor(h/2.0)-1.0));
  switch ((int) floor(h))
  {
    case 1: red=kQR*(mn+x); green=kQR*(mn+c); blue=kQR*mn; break;
    case 2: red=kQR*mn; green=kQR*(mn+c); blue=kQR*(mn+x); break;
    case 3: red=kQR*mn; green=kQR*(mn+x); blue=kQR*(mn+c); break;
    case 4: red=kQR*(mn+x); green=kQR*mn; blue=kQR*(mn+c); break;
    case 5: red=kQR*(mn+c); green=kQR*mn; blue=kQR*(mn+x); break;
    default: red=kQR*(mn+c); green=kQR*(mn+x); blue=kQR*mn; break;       // 0
  }
}

constexpr double kPi=3.1415926535897932384626433832795028841971693993751058209749445923078164062;   // MagickPI

} // namespace mh
