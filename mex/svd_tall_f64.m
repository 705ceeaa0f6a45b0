function [U, S, V, rank, converged] = svd_tall_f64(A, n_keep)
% [U,S,V] = svd(A,'econ') in float64 on the MI355X for min(size) <= 64 and a long side up to 65536 (jstsp_svd_tall_f64): the
% results and conventions of svd_f64 by a QR route - a streaming Householder reduction to the n x n triangle with the reflectors
% kept, one-sided Jacobi with vectors on the triangle, the reflectors applied back.  A = U*S*V' with S the n x n diagonal matrix
% (or its leading n_keep rows and columns); s = svd_tall_f64(A) returns the column of singular values.  A third array dimension
% is the batch.  rank: the singular values pinv's drop rule keeps (the long-side factor has zero columns from there on);
% converged: 0 where the sweep cap ended the iteration.
if nargin < 2
    n_keep = min(size(A, 1), size(A, 2));
end
if nargout <= 1
    U = jstsp_mex('svd_tall_f64', A, n_keep);
elseif nargout == 2
    [U, S] = jstsp_mex('svd_tall_f64', A, n_keep);
elseif nargout == 3
    [U, S, V] = jstsp_mex('svd_tall_f64', A, n_keep);
else
    [U, S, V, rank, converged] = jstsp_mex('svd_tall_f64', A, n_keep);
end
end
