// What apply.hip's tqr_lstsq takes from solve.hip besides the public tqr_trsm_r (include/tqr.h).
#pragma once

namespace tqr {

// dres[c] <- the 2-norm of rows n .. m-1 of column c of the m x nrhs device matrix dB (elements and
// result of `dtype`), c < nrhs; one launch on `stream`. Arguments are the caller's, already checked.
int resnorm(int dtype, const void* dB, int lddb, int n, int m, int nrhs, void* dres, void* stream);

}  // namespace tqr
