// The forward plan between Python dicts and gale/forward_plan.h: one field list per op kind
// (plan_dict.cpp), read strictly - a missing key, an unknown key or a list of the wrong length is
// a ValueError naming the op, its kind and the key - and written back in the same form.
#pragma once
#include <pybind11/pybind11.h>

#include <vector>

#include "gale/forward_plan.h"

namespace gale {

// A ConvDesc from the dict the kernel bindings take (conv2d, conv_mfma_plan, ...): the optional
// fields default, keys that are no ConvDesc field are ignored. Inside a plan op they are refused.
ConvDesc desc_from_dict(const pybind11::dict& d);

PlanSpec plan_spec_from_py(const pybind11::list& ops, std::vector<long long> buf_bytes,
                           int max_batch, int slots, std::vector<int> buckets, int chunk_ops,
                           int chunk_images);
// The ops as dicts with every key present (what build_plan writes).
pybind11::list plan_ops_to_py(const PlanSpec& spec);

}  // namespace gale
