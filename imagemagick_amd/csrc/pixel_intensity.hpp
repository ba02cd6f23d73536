// GetPixelIntensity (MagickCore/pixel.c:2356-2455) and the sRGB transfer functions it needs
// (pixel.c:260-451), restated for the device.  Shared by the kernels that weigh pixels by their
// intensity: Grayscale (pointwise.hip), Histogram and ContrastStretch (histogram.hip), pixel
// export (pixel_io.hip), the *Intensity morphology methods (morphology.hip), the threshold
// operators (threshold.hip), BilateralBlur and SelectiveBlur (edge_blur.hip), and by the
// colourspace kernels (colorspace.hip, colour_math.hpp) for the transfer functions.
#pragma once

#include "mh_internal.hpp"
#include "device_common.hpp"

namespace mh {

// --------------------------------------------------------------- sRGB gamma
// x^2.4 via frexp + 9-term Chebyshev + power-of-two table, pixel.c:260-316
static __device__ double decode_gamma(double x)
{
  const double c0=1.7917488588043277509,c1=0.82045614371976854984,
    c2=0.027694100686325412819,c3=-0.00094244335181762134018,
    c4=0.000064355540911469709545,c5=-5.7224404636060757485e-06,
    c6=5.8767669437311184313e-07,c7=-6.6139920053589721168e-08,
    c8=7.9323242696227458163e-09;
  int exponent;
  double t0=1.0;
  double t1=4.0*frexp(x,&exponent)-3.0;
  double t2=2.0*t1*t1-t0;
  double t3=2.0*t1*t2-t1;
  double t4=2.0*t1*t3-t2;
  double t5=2.0*t1*t4-t3;
  double t6=2.0*t1*t5-t4;
  double t7=2.0*t1*t6-t5;
  double t8=2.0*t1*t7-t6;
  double p=c0*t0+c1*t1+c2*t2+c3*t3+c4*t4+c5*t5+c6*t6+c7*t7+c8*t8;
  int e=exponent-1;
  int quot=e/5,rem=e%5;            // div(): truncation toward zero
  if (rem < 0)
    {
      quot-=1;
      rem+=5;
    }
  double pw;
  switch (rem)
  {
    case 0: pw=1.0; break;
    case 1: pw=2.6390158215457883983; break;
    case 2: pw=6.9644045063689921093; break;
    case 3: pw=1.8379173679952558018e+01; break;
    default: pw=4.8502930128332728543e+01; break;
  }
  return x*ldexp(pw*p,7*quot);
}

// x^(5/12), pixel.c:380-443
static __device__ double encode_gamma(double x)
{
  const double c0=1.1758200232996901923,c1=0.16665763094889061230,
    c2=-0.0083154894939042125035,c3=0.00075187976780420279038,
    c4=-0.000083240178519391795367,c5=0.000010229209410070008679,
    c6=-1.3400466409860246e-06,c7=1.8333422241635376682e-07,
    c8=-2.5878596761348859722e-08;
  int exponent;
  double t0=1.0;
  double t1=4.0*frexp(x,&exponent)-3.0;
  double t2=2.0*t1*t1-t0;
  double t3=2.0*t1*t2-t1;
  double t4=2.0*t1*t3-t2;
  double t5=2.0*t1*t4-t3;
  double t6=2.0*t1*t5-t4;
  double t7=2.0*t1*t6-t5;
  double t8=2.0*t1*t7-t6;
  double p=c0*t0+c1*t1+c2*t2+c3*t3+c4*t4+c5*t5+c6*t6+c7*t7+c8*t8;
  int e=exponent-1;
  int quot=e/12,rem=e%12;
  if (rem < 0)
    {
      quot-=1;
      rem+=12;
    }
  double pw;
  switch (rem)
  {
    case 0: pw=1.0; break;
    case 1: pw=1.3348398541700343678; break;
    case 2: pw=1.7817974362806785482; break;
    case 3: pw=2.3784142300054420538; break;
    case 4: pw=3.1748021039363991669; break;
    case 5: pw=4.2378523774371812394; break;
    case 6: pw=5.6568542494923805819; break;
    case 7: pw=7.5509945014535482244; break;
    case 8: pw=1.0079368399158985525e1; break;
    case 9: pw=1.3454342644059433809e1; break;
    case 10: pw=1.7959392772949968275e1; break;
    default: pw=2.3972913230026907883e1; break;
  }
  return ldexp(pw*p,5*quot);
}

// DecodePixelGamma, pixel.c:318-324
static __device__ double decode_pixel_gamma(double pixel)
{
  if (pixel <= (0.0404482362771076*kQR))
    return pixel/12.92;
  return kQR*decode_gamma((double) (kQS*pixel+0.055)/1.055);
}

// EncodePixelGamma, pixel.c:445-451
static __device__ double encode_pixel_gamma(double pixel)
{
  if (pixel <= (0.0031306684425005883*kQR))
    return 12.92*pixel;
  return kQR*(1.055*encode_gamma(kQS*pixel)-0.055);
}

// ---------------------------------------------------------------- intensity
struct IntensityParams
{
  int method;        // MhIntensityMethod
  int linear;        // colourspace is linear RGB / LinearGRAY
  int nonlinear;     // colourspace is sRGB / GRAY
  int gray;          // R,G,B all live at offset 0 (GRAY / LinearGRAY image)
};

// GetPixelIntensity, pixel.c:2356-2455
template<typename Q,int C>
static __device__ __forceinline__ double pixel_intensity(const Q (&q)[C],const IntensityParams &ip)
{
  double red=(double) q[0];
  if (C == 1)
    return red;
  double green=(double) q[(C >= 3) && !ip.gray ? 1 : 0];
  double blue=(double) q[(C >= 3) && !ip.gray ? 2 : 0];
  switch (ip.method)
  {
    case MH_INTENSITY_AVERAGE:
      return (red+green+blue)/3.0;
    case MH_INTENSITY_BRIGHTNESS:
    {
      double m=red > green ? red : green;
      return m > blue ? m : blue;
    }
    case MH_INTENSITY_LIGHTNESS:
    {
      double mn=red < green ? red : green;
      mn=mn < blue ? mn : blue;
      double mx=red > green ? red : green;
      mx=mx > blue ? mx : blue;
      return (mn+mx)/2.0;
    }
    case MH_INTENSITY_MS:
      return (red*red+green*green+blue*blue)/(3.0*kQR);
    case MH_INTENSITY_REC601LUMA:
      if (ip.linear)
        {
          red=encode_pixel_gamma(red);
          green=encode_pixel_gamma(green);
          blue=encode_pixel_gamma(blue);
        }
      return 0.298839*red+0.586811*green+0.114350*blue;
    case MH_INTENSITY_REC601LUMINANCE:
      if (ip.nonlinear)
        {
          red=decode_pixel_gamma(red);
          green=decode_pixel_gamma(green);
          blue=decode_pixel_gamma(blue);
        }
      return 0.298839*red+0.586811*green+0.114350*blue;
    case MH_INTENSITY_REC709LUMINANCE:
      if (ip.nonlinear)
        {
          red=decode_pixel_gamma(red);
          green=decode_pixel_gamma(green);
          blue=decode_pixel_gamma(blue);
        }
      return 0.212656*red+0.715158*green+0.072186*blue;
    case MH_INTENSITY_RMS:
      return sqrt(red*red+green*green+blue*blue)/sqrt(3.0);
    default:
      break;
  }
  if (ip.linear)
    {
      red=encode_pixel_gamma(red);
      green=encode_pixel_gamma(green);
      blue=encode_pixel_gamma(blue);
    }
  return 0.212656*red+0.715158*green+0.072186*blue;
}

static IntensityParams intensity_params(const MhImage *desc)
{
  IntensityParams ip;
  ip.method=(int) desc->intensity;
  ip.linear=(desc->colorspace == MH_COLORSPACE_RGB) || (desc->colorspace == MH_COLORSPACE_LINEARGRAY);
  ip.nonlinear=(desc->colorspace == MH_COLORSPACE_SRGB) || (desc->colorspace == MH_COLORSPACE_GRAY);
  ip.gray=(desc->colorspace == MH_COLORSPACE_GRAY) || (desc->colorspace == MH_COLORSPACE_LINEARGRAY) ||
    (desc->number_channels < 3);
  return ip;
}

// The default method on a frame that needs no gamma step (Rec709Luma of sRGB, Lab ... pixels),
// pixel.c:2446-2454 — three products and two sums, against the whole switch above inlined at
// every call site (the packed-table kernels evaluate 16 pixels per thread and step: 67 000
// instructions of ISA with the switch, and an instruction-cache-bound loop).
static bool intensity_is_plain_luma(const IntensityParams &ip,int channels)
{
  switch (ip.method)
  {
    case MH_INTENSITY_AVERAGE: case MH_INTENSITY_BRIGHTNESS: case MH_INTENSITY_LIGHTNESS: case MH_INTENSITY_MS:
    case MH_INTENSITY_REC601LUMA: case MH_INTENSITY_REC601LUMINANCE: case MH_INTENSITY_REC709LUMINANCE:
    case MH_INTENSITY_RMS:
      return false;
    default:
      break;
  }
  return (channels >= 3) && (ip.linear == 0) && (ip.gray == 0);
}

template<typename Q,int C>
static __device__ __noinline__ double pixel_intensity_call(const Q (&q)[C],const IntensityParams &ip)
{
  return pixel_intensity<Q,C>(q,ip);
}

template<bool PLAIN,typename Q,int C>
static __device__ __forceinline__ double pixel_intensity_of(const Q (&q)[C],const IntensityParams &ip)
{
  if constexpr (PLAIN && (C >= 3))
    return 0.212656*(double) q[0]+0.715158*(double) q[1]+0.072186*(double) q[2];
  else
    return pixel_intensity_call<Q,C>(q,ip);
}

} // namespace mh
