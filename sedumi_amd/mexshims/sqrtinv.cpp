// y = sqrtinv(q,vlab,K)  -- replaces sqrtinv.c:95-145 (updtransfo.m:103)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 3) mexErrMsgTxt("sqrtinv requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("sqrtinv generates less output arguments.");
  ConeK ck; read_cone(prhs[2], ck);
  sdm_int lenud = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) lenud += (k < ck.K.rsdpN ? 1 : 2) * ck.K.sdpNL[k] * ck.K.sdpNL[k];
  if ((sdm_int)numel(prhs[0]) != lenud) mexErrMsgTxt("q size mismatch");                 // sqrtinv.c:121
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_sqrtinv(&ck.K, mxGetPr(prhs[0]), mxGetPr(prhs[1]), (sdm_int)numel(prhs[1]), mxGetPr(plhs[0])));   // (:120 "v size mismatch" inside)
}
