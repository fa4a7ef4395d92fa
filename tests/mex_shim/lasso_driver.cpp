// lasso_driver.cpp -- calls the mexFunction of matlab/epiekf_pipeline_mex.cpp (compiled with -DmexFunction=mex_pipeline)
// with up to 16 outputs and writes them in order (tests/test_lasso_mex.py: the 'lasso' command returns 10).
//   lasso_driver <in.bin> <out.bin> <nlhs>
// File format as tests/mex_shim/driver.cpp: int32 count, then per array { int32 class (6 double, 12 int32, 4 char),
// int32 ndim, int64 dims[ndim], raw column-major data }.  A MEX error exits with status 3 and "MEXERROR[id]: text".
#include "mex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
extern "C" void mex_pipeline(int, mxArray *[], int, const mxArray *[]);

static size_t esz(int c) { return c == mxDOUBLE_CLASS ? 8 : c == mxINT32_CLASS ? 4 : 1; }

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: lasso_driver <in> <out> <nlhs>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("in"); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    std::vector<const mxArray *> prhs;
    for (int k = 0; k < count; k++) {
        int32_t cls, nd;
        if (fread(&cls, 4, 1, f) != 1 || fread(&nd, 4, 1, f) != 1) return 2;
        std::vector<mwSize> dims((size_t)nd);
        for (int i = 0; i < nd; i++) { int64_t v; if (fread(&v, 8, 1, f) != 1) return 2; dims[(size_t)i] = (mwSize)v; }
        mxArray *a = mxCreateNumericArray((mwSize)nd, dims.data(), (mxClassID)cls, mxREAL);
        const size_t bytes = mxGetNumberOfElements(a) * esz(cls);
        if (bytes && fread(mxGetData(a), 1, bytes, f) != bytes) return 2;
        prhs.push_back(a);
    }
    fclose(f);
    const int nlhs = atoi(argv[3]);
    if (nlhs < 1 || nlhs > 16) { fprintf(stderr, "nlhs must be 1 .. 16\n"); return 2; }
    mxArray *plhs[16] = {nullptr};
    try {
        mex_pipeline(nlhs, plhs, (int)prhs.size(), prhs.data());
    } catch (const MexError &e) {
        fprintf(stderr, "MEXERROR[%s]: %s\n", e.id.c_str(), e.msg.c_str());
        mxShimRunAtExit();
        return 3;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    int32_t n = 0;
    while (n < nlhs && plhs[n]) n++;
    fwrite(&n, 4, 1, o);
    for (int i = 0; i < n; i++) {
        const mxArray *a = plhs[i];
        const int32_t cls = mxShimClass(a), nd = (int32_t)mxGetNumberOfDimensions(a);
        fwrite(&cls, 4, 1, o); fwrite(&nd, 4, 1, o);
        for (int k = 0; k < nd; k++) { const int64_t v = (int64_t)mxGetDimensions(a)[k]; fwrite(&v, 8, 1, o); }
        const size_t bytes = mxGetNumberOfElements(a) * esz(cls);
        if (bytes) fwrite(mxGetData(a), 1, bytes, o);
    }
    fclose(o);
    mxShimRunAtExit();        // what `clear mex` does
    return 0;
}
