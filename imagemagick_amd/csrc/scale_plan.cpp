// Host plans of ScaleImage and SampleImage: see scale_plan.hpp.
#include "scale_plan.hpp"
#include "mh_internal.hpp"

namespace mh {

// resize.c:4196-4199, :4262-4372.  x_vector holds the row read last: when the source is exhausted
// (number_rows == image->rows) or next_row is false, the terms reuse it.
static void plan_rows(ScaleAxisPlan &plan)
{
  const size_t S=plan.source,D=plan.destination;
  size_t number_rows=0;
  bool next_row=true;
  double span=1.0;
  double scale=(double) D/(double) S;
  int32_t row=-1;                                   // the row in x_vector
  plan.start.assign(1,0u);
  for (size_t y=0; y < D; y++)
    {
      while (scale < span)
        {
          if (next_row && (number_rows < S))
            {
              row++;
              number_rows++;
            }
          plan.index.push_back(row);                // y_vector+=scale.y*x_vector
          plan.weight.push_back(scale);
          span-=scale;
          scale=(double) D/(double) S;
          next_row=true;
        }
      if (next_row && (number_rows < S))
        {
          row++;
          number_rows++;
          next_row=false;
        }
      plan.index.push_back(row);                    // pixel=y_vector+span.y*x_vector
      plan.weight.push_back(span);
      scale-=span;
      if (scale <= 0)
        {
          scale=(double) D/(double) S;
          next_row=true;
        }
      span=1.0;
      plan.start.push_back((uint32_t) plan.index.size());
    }
}

// resize.c:4419-4471.  pixel[] is the running sum; a store to scale_scanline[t] keeps the sum so far,
// and what is added after the last store of a column never reaches it.
static void plan_columns(ScaleAxisPlan &plan)
{
  const size_t S=plan.source,D=plan.destination;
  std::vector<int32_t> index;
  std::vector<double> weight;
  std::vector<size_t> begin(D,0),stored(D,0);        // per destination column: first term, terms at the last store
  bool next_column=false;
  double span=1.0;
  size_t t=0;
  bool in_range=true;
  // pixel[i]=0.0; t++
  const auto reset=[&]()
  {
    if (t < D)
      {
        index.resize(begin[t]+stored[t]);
        weight.resize(begin[t]+stored[t]);
      }
    t++;
    if (t < D)
      begin[t]=index.size();
  };
  const auto add=[&](size_t x,double w)
  {
    if (t < D)
      {
        index.push_back((int32_t) x);
        weight.push_back(w);
      }
  };
  const auto store=[&]()
  {
    if (t < D)
      stored[t]=index.size()-begin[t];
    else
      in_range=false;                                // scale_scanline[t] beyond the scanline
  };
  for (size_t x=0; x < S; x++)
    {
      double scale=(double) D/(double) S;
      while (scale >= span)
        {
          if (next_column)
            reset();
          add(x,span);
          store();
          scale-=span;
          span=1.0;
          next_column=true;
        }
      if (scale > 0)
        {
          if (next_column)
            {
              reset();
              next_column=false;
            }
          add(x,scale);
          span-=scale;
        }
    }
  if (span > 0)
    add(S-1,span);
  if (!next_column && (t < D))
    store();
  if (t < D)
    {
      index.resize(begin[t]+stored[t]);
      weight.resize(begin[t]+stored[t]);
    }
  plan.valid=in_range;
  plan.start.assign(1,0u);
  for (size_t d=0; d < D; d++)
    {
      if ((d > t) || (stored[d] == 0))
        {
          plan.valid=false;                          // a column the reference never stores
          break;
        }
      plan.start.push_back((uint32_t) (begin[d]+stored[d]));
    }
  if (!plan.valid)
    return;
  plan.index.swap(index);
  plan.weight.swap(weight);
}

ScaleAxisPlan scale_axis_plan(size_t source,size_t destination,int axis)
{
  ScaleAxisPlan plan;
  plan.source=source;
  plan.destination=destination;
  if ((source == 0) || (destination == 0) || (source > 0x3fffffffu) || (destination > 0x3fffffffu))
    {
      plan.valid=false;
      return plan;
    }
  if (source == destination)
    {
      plan.identity=true;
      plan.start.assign(destination+1,0u);
      return plan;
    }
  if (axis == 0)
    plan_rows(plan);
  else
    plan_columns(plan);
  if (!plan.valid)
    return plan;
  // the kernels stage the sources of a run of destinations as one interval: sources in visiting order
  for (size_t k=0; k < plan.index.size(); k++)
    if ((plan.index[k] < 0) || ((size_t) plan.index[k] >= source) || ((k > 0) && (plan.index[k] < plan.index[k-1])))
      plan.valid=false;
  for (size_t d=0; d < destination; d++)
    {
      const size_t terms=plan.start[d+1]-plan.start[d];
      plan.longest=terms > plan.longest ? terms : plan.longest;
    }
  return plan;
}

bool sample_offsets(size_t source,size_t destination,double percent,std::vector<long long> &offsets)
{
  offsets.clear();
  if ((source == 0) || (destination == 0) || (percent > 100.0) || (percent != percent))
    return false;
  // resize.c:3952, :3969
  const double offset=percent < 0.0 ? 0.5-kMagickEpsilon : percent/100.0-kMagickEpsilon;
  offsets.resize(destination);
  for (size_t j=0; j < destination; j++)
    {
      const double position=(((double) j+offset)*(double) source)/(double) destination;
      if (!(position > -1.0) || !(position < (double) source))
        return false;
      offsets[j]=(long long) position;
    }
  return true;
}

} // namespace mh

using namespace mh;

extern "C" {

MH_API long long MhScaleImagePlan(size_t source,size_t destination,int axis,unsigned *counts,int *indices,
  double *weights,size_t capacity)
{
  if ((source == 0) || (destination == 0) || ((axis != 0) && (axis != 1)))
    return -1;
  const ScaleAxisPlan plan=scale_axis_plan(source,destination,axis);
  if (!plan.valid)
    return -2;
  if (counts != nullptr)
    for (size_t d=0; d < destination; d++)
      counts[d]=plan.start[d+1]-plan.start[d];
  for (size_t k=0; (k < plan.index.size()) && (k < capacity); k++)
    {
      if (indices != nullptr)
        indices[k]=plan.index[k];
      if (weights != nullptr)
        weights[k]=plan.weight[k];
    }
  return (long long) plan.index.size();
}

MH_API int MhSampleImageOffsets(size_t source,size_t destination,double offset_percent,long long *offsets)
{
  std::vector<long long> table;
  if (!sample_offsets(source,destination,offset_percent,table))
    return -1;
  if (offsets != nullptr)
    for (size_t j=0; j < destination; j++)
      offsets[j]=table[j];
  return 0;
}

} // extern "C"
