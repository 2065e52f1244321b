// What the translation units of the plan builder share (plan.cpp, plan_fused.cpp, plan_chain_jit.cpp); not part of plan.hpp's interface.
#pragma once
#include "plan.hpp"

namespace gaast {

// plan_fused.cpp.  Whole-plan fusion for small programs: replaces the plan's steps with one FUSED step (true), or changes nothing.
bool try_fuse(Plan& plan, bool small_reg_slab);
// ... the slab size that fused plan would have; 0: the plan cannot be fused
int fused_slab(const Plan& plan, bool small_reg_slab);

// plan_chain_jit.cpp.  The list chain of step `c` (second list) and `wp` (first list) as a hiprtc-specialised kernel: fills c.cj, or
// leaves c.cj.on = 0.  wp == nullptr: a single list; init_off: the offsets of the covering copy folded into it.
void make_chain_jit(const Plan& plan, Step& c, const Step* wp, int64_t l1, int64_t r1, int64_t mid, int64_t r2, int alias, int side, bool covered,
                    const std::vector<uint32_t>* init_off = nullptr);

}  // namespace gaast
