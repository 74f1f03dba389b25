// z = psdjmul(x,y,K)  -- replaces psdjmul.m:40-73 (wregion.m's corrector); a MEX file of this name shadows the .m file
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 3) mexErrMsgTxt("psdjmul requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("psdjmul generates 1 output argument.");
  ConeK ck; read_cone(prhs[2], ck);
  if (ck.K.sdpN == 0) { plhs[0] = mxCreateDoubleMatrix(0, 0, mxREAL); return; }          // psdjmul.m:41-44: z = []
  sdm_int lenud = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) lenud += (k < ck.K.rsdpN ? 1 : 2) * ck.K.sdpNL[k] * ck.K.sdpNL[k];
  if (mxIsSparse(prhs[0]) || mxIsSparse(prhs[1])) mexErrMsgTxt("Sparse inputs not supported by this version of psdjmul.");
  const sdm_int len = (sdm_int)numel(prhs[0]);
  if ((sdm_int)numel(prhs[1]) != len || len < lenud) mexErrMsgTxt("psdjmul: size mismatch");       // :50: the last lenud entries of both
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_psdjmul(&ck.K, mxGetPr(prhs[0]), mxGetPr(prhs[1]), len, mxGetPr(plhs[0])));
}
