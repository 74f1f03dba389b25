// mineig = minpsdeig(x,K)  -- replaces minpsdeig.m:40-75 (maxstep.m:63); a MEX file of this name shadows the .m file
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 2) mexErrMsgTxt("minpsdeig requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("minpsdeig generates 1 output argument.");
  ConeK ck; read_cone(prhs[1], ck);
  if (ck.K.sdpN == 0) { plhs[0] = mxCreateDoubleMatrix(0, 0, mxREAL); return; }          // minpsdeig.m:47-50: mineig = []
  sdm_int lenud = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) lenud += (k < ck.K.rsdpN ? 1 : 2) * ck.K.sdpNL[k] * ck.K.sdpNL[k];
  if (mxIsSparse(prhs[0])) mexErrMsgTxt("Sparse inputs not supported by this version of minpsdeig.");
  const sdm_int len = (sdm_int)numel(prhs[0]);
  if (len < lenud) mexErrMsgTxt("minpsdeig: size mismatch");                               // :55: the last lenud entries
  plhs[0] = mxCreateDoubleMatrix(1, 1, mxREAL);
  int info = -1;
  sdm_check(sdm_minpsdeig(&ck.K, mxGetPr(prhs[0]), len, mxGetPr(plhs[0]), &info));
}
