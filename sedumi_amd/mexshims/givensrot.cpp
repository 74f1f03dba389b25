// y = givensrot(gjc,g,x,K)  -- replaces givensrot.c:93-168 (updtransfo.m:102)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 4) mexErrMsgTxt("givensrot requires more input arguments.");
  if (nlhs > 1) mexErrMsgTxt("givensrot generates less output arguments.");
  ConeK ck; read_cone(prhs[3], ck);
  sdm_int lenud = 0, slen = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) {
    const sdm_int n = ck.K.sdpNL[k];
    lenud += (k < ck.K.rsdpN ? 1 : 2) * n * n; slen += n;
  }
  if ((sdm_int)mxGetM(prhs[2]) != lenud || (lenud != 0 && mxGetN(prhs[2]) != 1)) mexErrMsgTxt("x size mismatch");   // givensrot.c:122
  if ((sdm_int)numel(prhs[0]) < slen) mexErrMsgTxt("gjc size mismatch");
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_givensrot(&ck.K, mxGetPr(prhs[0]), mxGetPr(prhs[1]), (sdm_int)numel(prhs[1]), mxGetPr(prhs[2]), mxGetPr(plhs[0])));
}
