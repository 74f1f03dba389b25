// x = psdframeit(lab,frms,K)  -- replaces psdframeit.c:107-168 (the PSD part of frameit.m:39)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 3) mexErrMsgTxt("psdframeit requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("psdframeit generates less output arguments.");
  ConeK ck; read_cone(prhs[2], ck);
  sdm_int lenud = 0, slen = 0, hlen = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) {
    const sdm_int n = ck.K.sdpNL[k];
    lenud += (k < ck.K.rsdpN ? 1 : 2) * n * n; slen += n; if (k >= ck.K.rsdpN) hlen += n;
  }
  const sdm_int lendiag = ck.K.lpN + 2 * ck.K.lorN + slen;
  const double *lab = mxGetPr(prhs[0]);
  if ((sdm_int)numel(prhs[0]) != slen) {                            // psdframeit.c:134-137
    if ((sdm_int)numel(prhs[0]) != lendiag) mexErrMsgTxt("lab size mismatch");
    lab += ck.K.lpN + 2 * ck.K.lorN;
  }
  if ((sdm_int)numel(prhs[1]) != lenud + hlen) mexErrMsgTxt("frms size mismatch");
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_psdframeit(&ck.K, lab, mxGetPr(prhs[1]), SDM_FRAME_HOUSEHOLDER, mxGetPr(plhs[0])));
}
