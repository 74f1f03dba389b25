// [u,perm,gjc,g] = urotorder(u,K,maxu,permIN)  -- replaces urotorder.c:312-490 (updtransfo.m:101)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 3) mexErrMsgTxt("urotorder requires more input arguments.");
  if (nlhs > 4) mexErrMsgTxt("urotorder generates less output arguments.");
  ConeK ck; read_cone(prhs[1], ck);
  sdm_int lenud = 0, slen = 0, gnnz = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) {
    const sdm_int n = ck.K.sdpNL[k];
    lenud += (k < ck.K.rsdpN ? 1 : 2) * n * n; slen += n; gnnz += (k < ck.K.rsdpN ? 2 : 3) * (n * (n - 1) / 2);
  }
  if ((sdm_int)numel(prhs[0]) != lenud) mexErrMsgTxt("u size mismatch");                 // urotorder.c:343
  const double *pin = NULL;
  if (nrhs >= 4 && numel(prhs[3]) > 0) {                                               // :346-351: optional, may be empty
    if ((sdm_int)numel(prhs[3]) != slen) mexErrMsgTxt("perm size mismatch");
    pin = mxGetPr(prhs[3]);
  }
  mxArray *out[3];
  out[0] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  out[1] = mxCreateDoubleMatrix(slen, 1, mxREAL);
  out[2] = mxCreateDoubleMatrix(slen, 1, mxREAL);
  std::vector<double> g((size_t)(gnnz > 0 ? gnnz : 1));
  sdm_int glen = 0;
  sdm_check(sdm_urotorder(&ck.K, mxGetPr(prhs[0]), mxGetScalar(prhs[2]), pin, mxGetPr(out[0]), mxGetPr(out[1]), mxGetPr(out[2]), g.data(), &glen));
  const int nout = nlhs > 1 ? nlhs : 1;
  for (int i = 0; i < 3; i++) {
    if (i < nout) plhs[i] = out[i];
    else mxDestroyArray(out[i]);
  }
  if (nout > 3) {                                                                      // :472-475: g is g_len x 1, 0 x 1 without a rotation
    plhs[3] = mxCreateDoubleMatrix(glen, 1, mxREAL);
    if (glen) memcpy(mxGetPr(plhs[3]), g.data(), (size_t)glen * sizeof(double));
  }
}
