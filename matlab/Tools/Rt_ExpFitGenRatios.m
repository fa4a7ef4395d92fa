function [Rt, Lambda, RtSmoothed, LambdaSmoothed] = Rt_ExpFitGenRatios(NewCases, wlen, generation_period, time_unit)
% Drop-in replacement of the reference's Tools/Rt_ExpFitGenRatios.m (same signature, same outputs): put this directory
% before the reference's Tools/ on the MATLAB path.  Runs on an MI355X through epiekf_rtwin_mex (DESIGN.md 4.4).
o = epiekf_rtwin_mex('GenRatios', NewCases(:)', wlen, generation_period, time_unit);
Rt = o.Rt; Lambda = o.Lambda; RtSmoothed = o.RtSmoothed; LambdaSmoothed = o.LambdaSmoothed;
end
