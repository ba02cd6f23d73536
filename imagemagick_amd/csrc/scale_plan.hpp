// Host plans of ScaleImage (MagickCore/resize.c:4106-4536) and SampleImage (:3907-4075).
//
// ScaleImage is serial in the reference: running accumulators across rows (y_vector, span.y,
// scale.y, next_row, number_rows) and across columns (pixel[], span.x, scale.x, next_column, t).  Both
// state machines depend on the four dimensions only, never on pixel data, so they are run here once
// per call and turn every destination sample into an ordered list of (source index, weight) terms.
// The weights are the doubles the reference's own statements produce, in its order; nothing is
// recomputed from a closed form.  Plain C++, no device code.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mh {

// One axis.  Destination sample d is  0.0 + w[k0]*s[i[k0]] + w[k0+1]*s[i[k0+1]] + ...  over
// k in [start[d], start[d+1]), every multiply and add separately rounded.  identity: source ==
// destination, the reference copies without arithmetic and there are no terms.
struct ScaleAxisPlan
{
  size_t source=0,destination=0;
  bool identity=false;
  // false: the reference would leave a destination column unset, store past its scanline, or (never
  // seen) visit sources out of order; the operator declines
  bool valid=true;
  std::vector<uint32_t> start;       // destination+1 entries
  std::vector<int32_t> index;
  std::vector<double> weight;
  size_t longest=0;                  // terms of the longest list
};

struct ScalePlan
{
  ScaleAxisPlan rows,columns;
};

// axis 0: rows (resize.c:4262-4372), axis 1: columns (:4411-4471)
ScaleAxisPlan scale_axis_plan(size_t source,size_t destination,int axis);

// SampleImage's x_offset / y_offset (resize.c:3984-3986, :4012).  percent < 0: the default offset.
// false: an offset leaves [0, source) or the percentage is above 100.
bool sample_offsets(size_t source,size_t destination,double percent,std::vector<long long> &offsets);

} // namespace mh
