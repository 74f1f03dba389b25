// [ux,ispos] = psdfactor(x,K)  -- replaces psdfactor.m:44-80 (trydif.m:62, widelen.m:101, wregion.m:62, :79); a MEX file of this
// name shadows the .m file
#include "mexcommon.h"
// ispos is a logical in MATLAB / Octave; the package's own MEX host (mexhost/mex.h) has full, sparse and struct arrays only: a 1 x 1 double there
static mxArray *ispos_value(bool v) {
#ifdef SDM_MEXHOST_MEX_H
  mxArray *a = mxCreateDoubleMatrix(1, 1, mxREAL);
  *mxGetPr(a) = v ? 1.0 : 0.0;
  return a;
#else
  return mxCreateLogicalScalar(v);
#endif
}
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 2) mexErrMsgTxt("psdfactor requires more input arguments.");
  if (nlhs > 2) mexErrMsgTxt("psdfactor generates 2 output arguments.");
  ConeK ck; read_cone(prhs[1], ck);
  sdm_int lenud = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) lenud += (k < ck.K.rsdpN ? 1 : 2) * ck.K.sdpNL[k] * ck.K.sdpNL[k];
  if (ck.K.sdpN == 0) {                                                                    // psdfactor.m:45-49: ux = zeros(0,1), ispos = true
    plhs[0] = mxCreateDoubleMatrix(0, 1, mxREAL);
    if (nlhs > 1) plhs[1] = ispos_value(true);
    return;
  }
  if (mxIsSparse(prhs[0])) mexErrMsgTxt("Sparse inputs not supported by this version of psdfactor.");
  const sdm_int len = (sdm_int)numel(prhs[0]);
  if (len < lenud) mexErrMsgTxt("psdfactor: size mismatch");                               // :55: the last lenud entries
  plhs[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  int ispos = 1;
  sdm_check(sdm_psdfactor(&ck.K, mxGetPr(prhs[0]), len, mxGetPr(plhs[0]), &ispos));
  if (nlhs > 1) plhs[1] = ispos_value(ispos != 0);
}
