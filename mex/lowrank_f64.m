function [X, tail] = lowrank_f64(A, R)
% The best rank-R approximation of A in the spectral and Frobenius norms, the leading R terms of svd_f64(A), computed and
% returned in float64 on the MI355X (jstsp_lowrank_f64).  tail = sigma_{R+1} = norm(A - X) (0 for R = min(size(A))).  A third
% array dimension is the batch: every page is approximated in ONE call, tail has one entry per page.
if nargout >= 2
    [X, tail] = jstsp_mex('lowrank_f64', A, R);
else
    X = jstsp_mex('lowrank_f64', A, R);
end
end
