// What apply.hip's tqr_lstsq and solve.hip's tqr_lstsq_fused share besides the public calls of
// include/tqr.h: the residual-norm launch (solve.hip) and a plan's shape (plans.hip).
#pragma once

struct tqr_plan;
struct tqr_solve;

namespace tqr {

// dres[c] <- the 2-norm of rows n .. m-1 of column c of the m x nrhs device matrix dB (elements and
// result of `dtype`), c < nrhs; one launch on `stream`. Arguments are the caller's, already checked.
int resnorm(int dtype, const void* dB, int lddb, int n, int m, int nrhs, void* dres, void* stream);

// The shape a plan was created for: m x n elements, tile size b, dtype, its steps (the cap of a
// tqr_plan_create_steps plan, else min(m, n) / b) and whether it came from tqr_plan_create_steps.
struct PlanShape {
  int m, n, b, dtype, steps;
  bool capped;
};
PlanShape plan_shape(const tqr_plan* pl);

// What a pipelined-solve handle was created for (solve_pipe.hip; read by apply_pipe.hip's tqr_lstsq_pipe).
struct SolveShape {
  int n, b, dtype, nrhs_max;
};
SolveShape solve_shape(const tqr_solve* sv);

}  // namespace tqr
