// [q,r] = qrK(x,K)  -- replaces qrK.c:236-296 (updtransfo.m:107, sdinit.m:86)
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs < 2) mexErrMsgTxt("qrK requires more input arguments");
  if (nlhs > 2) mexErrMsgTxt("qrK produces less output arguments");
  ConeK ck; read_cone(prhs[1], ck);
  sdm_int lenud = 0, hlen = 0;
  for (sdm_int k = 0; k < ck.K.sdpN; k++) {
    const sdm_int n = ck.K.sdpNL[k];
    lenud += (k < ck.K.rsdpN ? 1 : 2) * n * n; if (k >= ck.K.rsdpN) hlen += n;
  }
  if ((sdm_int)numel(prhs[0]) != lenud) mexErrMsgTxt("size mismatch x");          // qrK.c:260: rDim + hDim
  plhs[0] = mxCreateDoubleMatrix(lenud + hlen, 1, mxREAL);
  if (nlhs > 1) plhs[1] = mxCreateDoubleMatrix(lenud, 1, mxREAL);
  sdm_check(sdm_qrk(&ck.K, mxGetPr(prhs[0]), SDM_FRAME_HOUSEHOLDER, mxGetPr(plhs[0]), nlhs > 1 ? mxGetPr(plhs[1]) : NULL));
}
