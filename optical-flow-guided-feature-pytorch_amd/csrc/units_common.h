// Device-side blocks that the units kernels share: the site a block works for, the channel group (part) that
// holds a channel, the widening of a 16-bit element.  A units kernel takes these three from here.  The kernels that keep a copy of their
// own, and why, are listed in DESIGN.md 8.10.  Internal linkage, device only.
#pragma once
#include "offk_common.h"
#include "offk_internal.h"

namespace offk {
namespace {

// ---- the site of a block --------------------------------------------------------------------------------------------------
// The sites of a grouped launch own consecutive block ranges, in ascending order: the last site whose first block the block has
// reached is the block's.
//
// OFFK_PICK_SITE(S, p, reached): declares S, the site, COPIED.  `reached` is an expression in i: has the block reached site i?
// Unrolled over the by-value kernarg array this is one scalar select chain per member that the kernel goes on to read (the others
// fall away), and the copy lives in SGPRs.  It loads the members of all nine sites first.  A macro, not a function: the parameter
// block handed to an inlined function by reference is copied to scratch memory first (176 to 688 bytes per lane in
// units_dx_kernel), and so is a site indexed at run time.
#define OFFK_PICK_SITE(S, p, reached)                         \
  auto S = (p).s[0];                                          \
  _Pragma("unroll") for (int i = 1; i < kNumSites; ++i)       \
    if (i < (p).nsites && (reached)) S = (p).s[i];
// OFFK_SITE_INDEX(si, p, bid): declares si, the site's INDEX, scalar; `p.s[si]` then loads one site's members (nine compares, one
// indexed scalar load per member: the short prologue that the kernels with short blocks want).
#define OFFK_SITE_INDEX(si, p, bid)                           \
  int si = 0;                                                 \
  _Pragma("unroll") for (int i = 1; i < kNumSites; ++i)       \
    if (i < (p).nsites && (bid) >= (p).s[i].blk_begin) si = i; \
  si = __builtin_amdgcn_readfirstlane(si);
// blocks of site i (S, where the kernel holds a copy of it) of a launch whose parameter block carries total_blocks
#define OFFK_SITE_BLOCKS(p, i, S) (((i) + 1 < (p).nsites ? (p).s[(i) + 1].blk_begin : (p).total_blocks) - (S).blk_begin)

// ---- the part of a channel ------------------------------------------------------------------------------------------------
// A site's map is up to four channel groups (the branch outputs of an Inception block that were never concatenated): part q
// holds cp[q] channels behind xp[q], every cp a multiple of 32, so a K-tile never straddles two parts.  part_at: the part that
// holds channel c -- its base, its channels, c's index inside it.  c is uniform across the block: scalar selects.
// The walk stands here twice, because hipcc compiles the two spellings to different scalar compares and a kernel keeps its
// instructions only with the spelling its own text had: the struct form for the kernels that declared (base, channels, index) with
// part 0 and walked on, the form on three references for the kernels whose `locate` lambda assigned them.  Same rule, same result.
struct Part { const float* xb; int cpart, kl; };
template <class Site>
__device__ __forceinline__ Part part_at(const Site& S, int c) {
  Part k{S.xp[0], S.cp[0], c};
  if (S.nparts > 1 && k.kl >= S.cp[0]) {
    k.kl -= S.cp[0]; k.xb = S.xp[1]; k.cpart = S.cp[1];
    if (S.nparts > 2 && k.kl >= S.cp[1]) {
      k.kl -= S.cp[1]; k.xb = S.xp[2]; k.cpart = S.cp[2];
      if (S.nparts > 3 && k.kl >= S.cp[2]) { k.kl -= S.cp[2]; k.xb = S.xp[3]; k.cpart = S.cp[3]; }
    }
  }
  return k;
}
template <class Site>
__device__ __forceinline__ void part_at(const Site& S, int c, const float*& xb, int& cpart, int& kl) {
  xb = S.xp[0]; cpart = S.cp[0]; kl = c;
  if (S.nparts > 1 && kl >= S.cp[0]) {
    kl -= S.cp[0]; xb = S.xp[1]; cpart = S.cp[1];
    if (S.nparts > 2 && kl >= S.cp[1]) {
      kl -= S.cp[1]; xb = S.xp[2]; cpart = S.cp[2];
      if (S.nparts > 3 && kl >= S.cp[2]) { kl -= S.cp[2]; xb = S.xp[3]; cpart = S.cp[3]; }
    }
  }
}

// ---- 16-bit elements ------------------------------------------------------------------------------------------------------
// An element (FT = kFeatBf16 / kFeatF16) widened to the exact fp32 value it stands for.  bf16 is the upper half of an fp32
// word; fp16 goes through the hardware conversion, which keeps subnormals.
template <int FT>
__device__ __forceinline__ float widen16(unsigned h) {   // h: the element in the low 16 bits, upper bits zero
  if (FT == kFeatBf16) return __uint_as_float(h << 16);
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}
template <int FT>
__device__ __forceinline__ float4 widen16x4(unsigned lo, unsigned hi) {   // four consecutive elements in two words
  if (FT == kFeatBf16)
    return make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u));
  return make_float4(widen16<FT>(lo & 0xffffu), widen16<FT>(lo >> 16), widen16<FT>(hi & 0xffffu), widen16<FT>(hi >> 16));
}

}  // namespace
}  // namespace offk
