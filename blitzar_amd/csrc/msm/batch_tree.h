// Montgomery's trick across T lanes (T a power of two), the parts that compile for the host as well:
// `tree` has 2 T entries in heap order (root 1, leaf T + lane).  A level of the product tree and a
// level of the way back down are one step per lane; msm/kernels.h (tree_products, tree_inverses)
// puts the workgroup barriers between the levels, tests/native/batch_normalise_check.cc runs the
// same steps lane after lane.
#pragma once

#include "blitzar_amd/csrc/base/macros.h"

namespace bz {

// level s (s = T / 2 down to 1): node s + tid becomes the product of its children
template <class C>
BZ_HD void tree_product_step(typename C::batch_fe* tree, u32 s, u32 tid) {
  if (tid < s) tree[s + tid] = C::batch_mul(tree[2 * (s + tid)], tree[2 * (s + tid) + 1]);
}
// level s (s = 1 up to T / 2), tree[1] holding the inverse of the root: the children of node s + tid
// become the inverses of their subtrees' products (inv * sibling)
template <class C>
BZ_HD void tree_inverse_step(typename C::batch_fe* tree, u32 s, u32 tid) {
  if (tid < s) {
    const u32 i = s + tid;
    const typename C::batch_fe inv = tree[i], left = tree[2 * i], right = tree[2 * i + 1];
    tree[2 * i] = C::batch_mul(inv, right);
    tree[2 * i + 1] = C::batch_mul(inv, left);
  }
}
// The leaf of a lane whose value may be zero mod p, or that has no value at all (`live` false): one()
// stands in, so that a single zero never reaches the shared product -- it would zero the inverse
// of every other leaf of the tree.  The lane gets 1 back as its "inverse".
template <class C>
BZ_HD typename C::batch_fe tree_leaf(const typename C::batch_fe& z, bool live) {
  return live && !C::batch_is_zero(z) ? z : C::batch_one();
}
} // namespace bz
