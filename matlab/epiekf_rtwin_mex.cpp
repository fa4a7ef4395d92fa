// epiekf_rtwin_mex.cpp -- MEX gateway for the sliding-window growth-rate estimators (epi_rtwin_run_host):
//   o = epiekf_rtwin_mex('LogLinReg', x, wlen, time_unit, causal)           -> o.Rt, o.A, o.Lambda, o.ExpFit
//   o = epiekf_rtwin_mex('GenRatios', x, wlen, generation_period, time_unit) -> o.Rt, o.Lambda, o.RtSmoothed, o.LambdaSmoothed
//   o = epiekf_rtwin_mex('NonlinLS',  x, wlen, time_unit, causal)           -> o.Rt, o.A, o.Lambda, o.ExpFit, o.status, o.iters
// x is R x L: one series per row (the drop-in wrappers in matlab/Tools/ pass NewCases(:)', R = 1).  MATLAB's column-major
// R x L array is the ABI's [L][R] layout, so it is passed straight through; every output is R x L (status / iters int32).
// NonlinLS raises 'epiekf:nlinfit' where nlinfit would (a window with status EPI_RTWIN_MODEL_ERROR).
// Build on a MATLAB host:  mex -I../include epiekf_rtwin_mex.cpp -L../epidemicmodeling_amd -lepiekf
#include <string.h>
#include "mex.h"
#include "epiekf.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 5) mexErrMsgTxt("epiekf_rtwin_mex: 5 inputs expected (method, x, and three scalars)");
    char method[32] = {0};
    if (mxGetString(prhs[0], method, sizeof method) != 0) mexErrMsgTxt("epiekf_rtwin_mex: the first input names the method");
    epi_rtwin_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION;
    d.R = (int32_t)mxGetM(prhs[1]);
    d.L = (int32_t)mxGetN(prhs[1]);
    d.wlen = (int32_t)mxGetScalar(prhs[2]);
    const char *const *names;
    int nout;
    static const char *const llr[] = {"Rt", "A", "Lambda", "ExpFit"};
    static const char *const gr[] = {"Rt", "Lambda", "RtSmoothed", "LambdaSmoothed"};
    static const char *const nls[] = {"Rt", "A", "Lambda", "ExpFit", "status", "iters"};
    if (!strcmp(method, "LogLinReg")) {
        d.methods = EPI_RTWIN_LOGLINREG; d.time_unit = mxGetScalar(prhs[3]); d.causal = (int32_t)mxGetScalar(prhs[4]);
        names = llr; nout = 4;
    } else if (!strcmp(method, "GenRatios")) {
        d.methods = EPI_RTWIN_GENRATIOS; d.generation_period = (int32_t)mxGetScalar(prhs[3]); d.time_unit = mxGetScalar(prhs[4]);
        d.causal = 1;
        names = gr; nout = 4;
    } else if (!strcmp(method, "NonlinLS")) {
        d.methods = EPI_RTWIN_NONLINLS; d.time_unit = mxGetScalar(prhs[3]); d.causal = (int32_t)mxGetScalar(prhs[4]);
        names = nls; nout = 6;
    } else {
        mexErrMsgIdAndTxt("epiekf:error", "epiekf_rtwin_mex: unknown method '%s'", method);
        return;
    }
    const mwSize dims[2] = {(mwSize)d.R, (mwSize)d.L};
    mxArray *v[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < nout; i++) v[i] = mxCreateNumericArray(2, dims, i < 4 ? mxDOUBLE_CLASS : mxINT32_CLASS, mxREAL);
    epi_rtwin_outputs out;
    memset(&out, 0, sizeof out);
    double *p[4] = {mxGetPr(v[0]), mxGetPr(v[1]), mxGetPr(v[2]), mxGetPr(v[3])};
    if (d.methods == EPI_RTWIN_LOGLINREG) { out.llr_Rt = p[0]; out.llr_A = p[1]; out.llr_Lambda = p[2]; out.llr_ExpFit = p[3]; }
    else if (d.methods == EPI_RTWIN_GENRATIOS) { out.gr_Rt = p[0]; out.gr_Lambda = p[1]; out.gr_RtSmoothed = p[2]; out.gr_LambdaSmoothed = p[3]; }
    else {
        out.nls_Rt = p[0]; out.nls_A = p[1]; out.nls_Lambda = p[2]; out.nls_ExpFit = p[3];
        out.nls_status = (int32_t *)mxGetData(v[4]); out.nls_iters = (int32_t *)mxGetData(v[5]);
    }
    char err[256] = {0};
    const int rc = epi_rtwin_run_host(&d, mxGetPr(prhs[1]), &out, /*device=*/0, err);
    if (rc != EPI_OK) mexErrMsgIdAndTxt("epiekf:error", "%s (%s)", err, epi_status_string(rc));
    if (d.methods == EPI_RTWIN_NONLINLS) {
        const size_t n = (size_t)d.R * (size_t)d.L;
        for (size_t k = 0; k < n; k++)
            if (out.nls_status[k] == EPI_RTWIN_MODEL_ERROR)
                mexErrMsgIdAndTxt("epiekf:nlinfit", "nlinfit fails in the window of series %d, day %d: the model returned Inf or "
                                  "NaN, or fewer than 2 samples remain", (int)(k % (size_t)d.R) + 1, (int)(k / (size_t)d.R) + 1);
    }
    plhs[0] = mxCreateStructMatrix(1, 1, nout, (const char **)names);
    for (int i = 0; i < nout; i++) mxSetFieldByNumber(plhs[0], 0, i, v[i]);
    (void)nlhs;
}
