// z = psdinvjmul(xlab,xfrm,y,K)  -- replaces psdinvjmul.c:165-227 (the PSD part of wregion.m:98)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 4) mexErrMsgTxt("psdinvjmul requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("psdinvjmul generates 1 output argument.");
  ConeK ck; read_cone(prhs[3], ck);
  sdm_int lenud = 0, slen = 0, hlen = 0, qdim = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) {
    const sdm_int n = ck.K.sdpNL[k];
    lenud += (k < ck.K.rsdpN ? 1 : 2) * n * n; slen += n; if (k >= ck.K.rsdpN) hlen += n;
  }
  for (sdm_int k = 0; k < ck.K.lorN; k++) qdim += ck.K.lorNL[k];
  const sdm_int lenfull = ck.K.lpN + qdim + lenud, lendiag = ck.K.lpN + 2 * ck.K.lorN + slen;
  if (mxIsSparse(prhs[0]) || mxIsSparse(prhs[2])) mexErrMsgTxt("Sparse inputs not supported by this version of psdinvjmul.");
  const double *x = mxGetPr(prhs[0]), *y = mxGetPr(prhs[2]);
  if ((sdm_int)numel(prhs[2]) != lenud) {                           // psdinvjmul.c:195-198
    if ((sdm_int)numel(prhs[2]) != lenfull) mexErrMsgTxt("size y mismatch.");
    y += ck.K.lpN + qdim;
  }
  if ((sdm_int)numel(prhs[0]) != slen) {                            // psdinvjmul.c:199-202
    if ((sdm_int)numel(prhs[0]) != lendiag) mexErrMsgTxt("size xlab mismatch.");
    x += ck.K.lpN + 2 * ck.K.lorN;
  }
  if ((sdm_int)numel(prhs[1]) != lenud + hlen) mexErrMsgTxt("size xfrm mismatch.");
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_psdinvjmul(&ck.K, x, mxGetPr(prhs[1]), SDM_FRAME_HOUSEHOLDER, y, mxGetPr(plhs[0])));
}
