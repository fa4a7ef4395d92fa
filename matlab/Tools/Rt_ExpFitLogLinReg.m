function [Rt, A, Lambda, ExpFit] = Rt_ExpFitLogLinReg(NewCases, wlen, time_unit, varargin)
% Drop-in replacement of the reference's Tools/Rt_ExpFitLogLinReg.m (same signature, same outputs): put this directory
% before the reference's Tools/ on the MATLAB path.  Runs on an MI355X through epiekf_rtwin_mex (DESIGN.md 4.4).
causal = 1;
if nargin > 3, causal = varargin{1}; end
o = epiekf_rtwin_mex('LogLinReg', NewCases(:)', wlen, time_unit, causal);
Rt = o.Rt; A = o.A; Lambda = o.Lambda; ExpFit = o.ExpFit;
end
