function [X, tail] = lowrank_tall_f64(A, R)
% The best rank-R approximation of A, the leading R terms of svd_tall_f64(A), in float64 on the MI355X for min(size) <= 64 and a
% long side up to 65536 (jstsp_lowrank_tall_f64).  tail = sigma_{R+1} = norm(A - X) (0 for R = min(size(A))).  A third array
% dimension is the batch: every page is approximated in ONE call, tail has one entry per page.
if nargout >= 2
    [X, tail] = jstsp_mex('lowrank_tall_f64', A, R);
else
    X = jstsp_mex('lowrank_tall_f64', A, R);
end
end
