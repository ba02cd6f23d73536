#!/usr/bin/env python3
"""Generates, at build time, copies of nine MagickCore sources with the accelerate call
sites the reference does not have (or has commented out) switched in — SURVEY 8b: "new hooks
for Morphology and Colorspace", the disabled UnsharpMask stanza, the caller-less
ContrastStretch, WaveletDenoise's hook without its softness argument — and a hook that
StatisticImage, BilateralBlurImage, SelectiveBlurImage, KuwaharaImage, CLAHEImage, AdaptiveThresholdImage, BilevelImage,
AutoThresholdImage, LevelImage, LevelizeImage, GammaImage, NegateImage, SigmoidalContrastImage, LinearStretchImage,
MinMaxStretchImage, SampleImage and ScaleImage lack altogether.  Each hook is the reference's own three-line idiom
(effect.c:783-787).  The copies are written under shim/_build/ (never committed, never
shipped); the reference tree is only read.

    python shim/patch_hooks.py <reference MagickCore dir> <output dir>
"""
import os
import sys

# entry points of shim/accelerate_hip.c that accelerate-private.h does not declare
MORPHOLOGY_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateMorphologyApply(const Image *,const MorphologyMethod,
  const ssize_t,const KernelInfo *,const CompositeOperator,const double,ExceptionInfo *);
#endif
'''
WAVELET_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateWaveletDenoiseImageSoft(const Image *,const double,
  const double,ExceptionInfo *);
#endif
'''
COLORSPACE_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate MagickBooleanType AccelerateTransformImageColorspace(Image *,
  const ColorspaceType,ExceptionInfo *);
#endif
'''

STATISTIC_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateStatisticImage(const Image *,const StatisticType,
  const size_t,const size_t,ExceptionInfo *);
#endif
'''

EFFECT_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateBilateralBlurImage(const Image *,const size_t,const size_t,
  const double,const double,ExceptionInfo *);
extern MagickPrivate Image *AccelerateSelectiveBlurImage(const Image *,const double,const double,
  const double,ExceptionInfo *);
extern MagickPrivate Image *AccelerateKuwaharaImage(const Image *,const double,const double,
  ExceptionInfo *);
#endif
'''

ENHANCE_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate MagickBooleanType AccelerateCLAHEImage(Image *,const size_t,const size_t,
  const size_t,const double,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateLevelImage(Image *,const double,const double,const double,
  ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateLevelizeImage(Image *,const double,const double,const double,
  ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateGammaImage(Image *,const double,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateNegateImage(Image *,const MagickBooleanType,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateSigmoidalContrastImage(Image *,const MagickBooleanType,
  const double,const double,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateLinearStretchImage(Image *,const double,const double,
  ExceptionInfo *);
#endif
'''

HISTOGRAM_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate MagickBooleanType AccelerateMinMaxStretchImage(Image *,const double,const double,
  const double,ExceptionInfo *);
#endif
'''

THRESHOLD_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateAdaptiveThresholdImage(const Image *,const size_t,const size_t,
  const double,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateBilevelImage(Image *,const double,ExceptionInfo *);
extern MagickPrivate MagickBooleanType AccelerateAutoThresholdImage(Image *,const AutoThresholdMethod,
  ExceptionInfo *);
#endif
'''

RESIZE_PROTOTYPE = '''
#if defined(MAGICKCORE_OPENCL_SUPPORT)
extern MagickPrivate Image *AccelerateSampleImage(const Image *,const size_t,const size_t,ExceptionInfo *);
extern MagickPrivate Image *AccelerateScaleImage(const Image *,const size_t,const size_t,ExceptionInfo *);
#endif
'''


def once(text, anchor, replacement, name):
    if text.count(anchor) != 1:
        raise SystemExit("%s: anchor %r found %d times" % (name, anchor, text.count(anchor)))
    return text.replace(anchor, replacement)


def after_includes(text, prototype):
    """Insert a prototype after the last #include of the leading include block."""
    marker = '#include "MagickCore/'
    last = text.rindex(marker, 0, text.index("\n/*\n", text.index(marker)))
    end = text.index("\n", last) + 1
    return text[:end] + prototype + text[end:]


def in_function(text, opening, anchor, replacement, name):
    """once(), within the function that `opening` starts."""
    begin = text.index(opening)
    end = text.index("\n}\n", begin)
    return text[:begin] + once(text[begin:end], anchor, replacement, name) + text[end:]


def morphology(text):
    text = after_includes(text, MORPHOLOGY_PROTOTYPE)
    anchor = "  count = 0;      /* number of low-level morphology primitives performed */\n"
    hook = anchor + '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  {
    Image *accelerated_image=AccelerateMorphologyApply(image,method,iterations,kernel,
      compose,bias,exception);
    if (accelerated_image != (Image *) NULL)
      return(accelerated_image);
  }
#endif
'''
    return once(text, anchor, hook, "morphology.c")


def effect(text):
    text = once(text, "/* This kernel appears to be broken.\n#if defined(MAGICKCORE_OPENCL_SUPPORT)\n  unsharp_image=AccelerateUnsharpMaskImage(",
                "#if defined(MAGICKCORE_OPENCL_SUPPORT)\n  unsharp_image=AccelerateUnsharpMaskImage(", "effect.c")
    text = once(text, "    return(unsharp_image);\n#endif\n*/\n", "    return(unsharp_image);\n#endif\n", "effect.c")
    # BilateralBlurImage and SelectiveBlurImage have no accelerate hook in the reference: one in
    # front of the first CloneImage of each (SelectiveBlurImage owns its kernel by then)
    text = after_includes(text, EFFECT_PROTOTYPE)
    anchor = "  blur_image=CloneImage(image,0,0,MagickTrue,exception);\n"
    text = in_function(text, "MagickExport Image *BilateralBlurImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  blur_image=AccelerateBilateralBlurImage(image,width,height,intensity_sigma,
    spatial_sigma,exception);
  if (blur_image != (Image *) NULL)
    return(blur_image);
#endif
''' + anchor, "effect.c")
    text = in_function(text, "MagickExport Image *SelectiveBlurImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  blur_image=AccelerateSelectiveBlurImage(image,radius,sigma,threshold,exception);
  if (blur_image != (Image *) NULL)
    {
      kernel=(MagickRealType *) RelinquishAlignedMemory(kernel);
      return(blur_image);
    }
#endif
''' + anchor, "effect.c")
    # KuwaharaImage has none either: one in front of its BlurImage, so that the whole operator, blur
    # included, runs on the device
    anchor = "  gaussian_image=BlurImage(image,radius,sigma,exception);\n"
    return in_function(text, "MagickExport Image *KuwaharaImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  kuwahara_image=AccelerateKuwaharaImage(image,radius,sigma,exception);
  if (kuwahara_image != (Image *) NULL)
    return(kuwahara_image);
#endif
''' + anchor, "effect.c")


def enhance(text):
    anchor = "  type=IdentifyImageType(image,exception);\n"
    hook = '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateContrastStretchImage(image,black_point,white_point,exception) != MagickFalse)
    return(MagickTrue);
#endif
''' + anchor
    begin = text.index("MagickExport MagickBooleanType ContrastStretchImage(")
    end = text.index("MagickExport", begin + 10)
    body = once(text[begin:end], anchor, hook, "enhance.c")
    text = text[:begin] + body + text[end:]
    # CLAHEImage has no accelerate hook in the reference: one at its top, in front of the tile
    # geometry, so that both colourspace transforms and the equalisation run on the device
    text = after_includes(text, ENHANCE_PROTOTYPE)
    anchor = "  range_info.min=0;\n"
    text = in_function(text, "MagickExport MagickBooleanType CLAHEImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateCLAHEImage(image,width,height,number_bins,clip_limit,exception) != MagickFalse)
    return(MagickTrue);
#endif
''' + anchor, "enhance.c")
    # The level operators have none either: one at the top of each, in front of the first statement
    # behind the asserts (GammaImage and SigmoidalContrastImage: behind their "nothing to do" return)
    colormap = "  if (image->storage_class == PseudoClass)\n"
    for function, anchor, call in (
            ("LevelImage(", colormap, "AccelerateLevelImage(image,black_point,white_point,gamma,exception)"),
            ("LevelizeImage(", colormap, "AccelerateLevelizeImage(image,black_point,white_point,gamma,exception)"),
            ("GammaImage(", "  gamma_map=(Quantum *) AcquireQuantumMemory(MaxMap+1UL,sizeof(*gamma_map));\n",
             "AccelerateGammaImage(image,gamma,exception)"),
            ("NegateImage(", colormap, "AccelerateNegateImage(image,grayscale,exception)"),
            ("SigmoidalContrastImage(", colormap,
             "AccelerateSigmoidalContrastImage(image,sharpen,contrast,midpoint,exception)"),
            ("LinearStretchImage(", "  histogram=(double *) AcquireQuantumMemory(MaxMap+1UL,sizeof(*histogram));\n",
             "AccelerateLinearStretchImage(image,black_point,white_point,exception)")):
        text = in_function(text, "MagickExport MagickBooleanType " + function, anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (%s != MagickFalse)
    return(MagickTrue);
#endif
''' % call + anchor, "enhance.c")
    return text


def colorspace(text):
    text = after_includes(text, COLORSPACE_PROTOTYPE)
    begin = text.index("MagickExport MagickBooleanType TransformImageColorspace(")
    end = text.index("\n}\n", begin)
    anchor = "  if (colorspace == UndefinedColorspace)\n    return(SetImageColorspace(image,colorspace,exception));\n"
    hook = anchor + '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateTransformImageColorspace(image,colorspace,exception) != MagickFalse)
    return(MagickTrue);
#endif
'''
    body = once(text[begin:end], anchor, hook, "colorspace.c")
    return text[:begin] + body + text[end:]


def visual_effects(text):
    # the reference's hook drops `softness`; pass it (the CPU result depends on it)
    text = after_includes(text, WAVELET_PROTOTYPE)
    return once(text, "  noise_image=AccelerateWaveletDenoiseImage(image,threshold,exception);\n",
                "  noise_image=AccelerateWaveletDenoiseImageSoft(image,threshold,softness,exception);\n",
                "visual-effects.c")


def statistic(text):
    # StatisticImage has no accelerate hook in the reference: one in front of its CloneImage
    text = after_includes(text, STATISTIC_PROTOTYPE)
    anchor = "  statistic_image=CloneImage(image,0,0,MagickTrue,\n    exception);\n"
    hook = '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  statistic_image=AccelerateStatisticImage(image,type,width,height,exception);
  if (statistic_image != (Image *) NULL)
    return(statistic_image);
#endif
''' + anchor
    return once(text, anchor, hook, "statistic.c")


def threshold(text):
    # AdaptiveThresholdImage, BilevelImage and AutoThresholdImage have no accelerate hook in the
    # reference: one at the top of each, in front of the first statement behind the asserts
    text = after_includes(text, THRESHOLD_PROTOTYPE)
    anchor = "  threshold_image=CloneImage(image,0,0,MagickTrue,exception);\n"
    text = in_function(text, "MagickExport Image *AdaptiveThresholdImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  threshold_image=AccelerateAdaptiveThresholdImage(image,width,height,bias,exception);
  if (threshold_image != (Image *) NULL)
    return(threshold_image);
#endif
''' + anchor, "threshold.c")
    anchor = "  if (SetImageStorageClass(image,DirectClass,exception) == MagickFalse)\n"
    text = in_function(text, "MagickExport MagickBooleanType BilevelImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateBilevelImage(image,threshold,exception) != MagickFalse)
    return(MagickTrue);
#endif
''' + anchor, "threshold.c")
    anchor = "  histogram=(double *) AcquireQuantumMemory(MaxIntensity+1UL,\n    sizeof(*histogram));\n"
    return in_function(text, "MagickExport MagickBooleanType AutoThresholdImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateAutoThresholdImage(image,method,exception) != MagickFalse)
    return(MagickTrue);
#endif
''' + anchor, "threshold.c")


def histogram(text):
    # MinMaxStretchImage (AutoLevelImage's body) has no accelerate hook in the reference: one at its top
    text = after_includes(text, HISTOGRAM_PROTOTYPE)
    anchor = "  status=MagickTrue;\n"
    return in_function(text, "MagickExport MagickBooleanType MinMaxStretchImage(", anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  if (AccelerateMinMaxStretchImage(image,black,white,gamma,exception) != MagickFalse)
    return(MagickTrue);
#endif
''' + anchor, "histogram.c")


def resize(text):
    # SampleImage and ScaleImage have no accelerate hook in the reference: one in front of the sized
    # CloneImage of each, behind the same-size early return.  ThumbnailImage needs none: its three
    # callees are SampleImage and ResizeImage, and its frame stays on the device between them.
    text = after_includes(text, RESIZE_PROTOTYPE)
    for function, result in (("SampleImage(", "sample_image"), ("ScaleImage(", "scale_image")):
        anchor = "  %s=CloneImage(image,columns,rows,MagickTrue,exception);\n" % result
        text = in_function(text, "MagickExport Image *" + function, anchor, '''#if defined(MAGICKCORE_OPENCL_SUPPORT)
  %s=Accelerate%simage,columns,rows,exception);
  if (%s != (Image *) NULL)
    return(%s);
#endif
''' % (result, function, result, result) + anchor, "resize.c")
    return text


def main():
    source, out = sys.argv[1], sys.argv[2]
    os.makedirs(out, exist_ok=True)
    for name, fn in (("morphology.c", morphology), ("effect.c", effect), ("enhance.c", enhance),
                     ("colorspace.c", colorspace), ("visual-effects.c", visual_effects),
                     ("statistic.c", statistic), ("threshold.c", threshold), ("histogram.c", histogram),
                     ("resize.c", resize)):
        text = open(os.path.join(source, name), encoding="latin-1").read()
        patched = fn(text)
        with open(os.path.join(out, name), "w", encoding="latin-1") as f:
            f.write('#line 1 "%s"\n' % os.path.join(source, name))
            f.write(patched)


if __name__ == "__main__":
    main()
