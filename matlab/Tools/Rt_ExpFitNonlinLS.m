function [Rt, A, Lambda, ExpFit] = Rt_ExpFitNonlinLS(NewCases, wlen, time_unit, varargin)
% Drop-in replacement of the reference's Tools/Rt_ExpFitNonlinLS.m (same signature, same outputs): put this directory
% before the reference's Tools/ on the MATLAB path.  Runs on an MI355X through epiekf_rtwin_mex; nlinfit's
% Levenberg-Marquardt as read in DESIGN.md 4.4.  Raises 'epiekf:nlinfit' where nlinfit raises.
causal = 1;
if nargin > 3, causal = varargin{1}; end
o = epiekf_rtwin_mex('NonlinLS', NewCases(:)', wlen, time_unit, causal);
Rt = o.Rt; A = o.A; Lambda = o.Lambda; ExpFit = o.ExpFit;
end
