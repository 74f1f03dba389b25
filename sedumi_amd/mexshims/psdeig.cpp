// [lab,q] = psdeig(x,K)  -- replaces psdeig.m:44-93 (wregion.m, updtransfo.m, trydif.m); a MEX file of this name shadows the .m file
#include "mexcommon.h"
#include <cmath>
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 2) mexErrMsgTxt("psdeig requires more input arguments.");
  if (nlhs > 2) mexErrMsgTxt("psdeig generates 2 output arguments.");
  ConeK ck; read_cone(prhs[1], ck);
  if (ck.K.sdpN == 0) {                                                                    // psdeig.m:43-46: lab = []
    plhs[0] = mxCreateDoubleMatrix(0, 0, mxREAL);
    if (nlhs > 1) plhs[1] = mxCreateDoubleMatrix(0, 0, mxREAL);
    return;
  }
  sdm_int lenud = 0, slen = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) { lenud += (k < ck.K.rsdpN ? 1 : 2) * ck.K.sdpNL[k] * ck.K.sdpNL[k]; slen += ck.K.sdpNL[k]; }
  if (mxIsSparse(prhs[0])) mexErrMsgTxt("Sparse inputs not supported by this version of psdeig.");
  const sdm_int len = (sdm_int)numel(prhs[0]);
  if (len < lenud) mexErrMsgTxt("psdeig: size mismatch");                                  // :51: the last lenud entries
  plhs[0] = mxCreateDoubleMatrix(slen, 1, mxREAL);
  if (nlhs > 1) plhs[1] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  int info = -1;
  sdm_check(sdm_psdeig(&ck.K, mxGetPr(prhs[0]), len, mxGetPr(plhs[0]), nlhs > 1 ? mxGetPr(plhs[1]) : NULL, &info));
  // a block that is not done comes back as NaN (an entry that is not finite, or no convergence): eig's own error is the caller's to raise
}
