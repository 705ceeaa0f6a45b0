function [U, S, V, rank, converged] = svd_f64(A, n_keep)
% [U,S,V] = svd(A,'econ') computed and returned in float64 on the MI355X (jstsp_svd_f64): one-sided Jacobi on the matrix itself,
% no Gram matrix; A = U*S*V' with S the n x n diagonal matrix, n = min(size(A,1), size(A,2)) (or its leading n_keep rows and
% columns).  s = svd_f64(A) returns the column of singular values.  A third array dimension is the batch: every page is
% decomposed in ONE call.  rank: the singular values pinv's drop rule keeps (the long-side factor has zero columns from there on);
% converged: 0 where the sweep cap ended the iteration.  min(size) <= 512, max(size) <= 8192.
if nargin < 2
    n_keep = min(size(A, 1), size(A, 2));
end
if nargout <= 1
    U = jstsp_mex('svd_f64', A, n_keep);
elseif nargout == 2
    [U, S] = jstsp_mex('svd_f64', A, n_keep);
elseif nargout == 3
    [U, S, V] = jstsp_mex('svd_f64', A, n_keep);
else
    [U, S, V, rank, converged] = jstsp_mex('svd_f64', A, n_keep);
end
end
