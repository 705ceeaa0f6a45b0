function [P, rcond, rank] = pinv_f64(A)
% MATLAB's pinv(A) computed and returned in float64 on the MI355X (jstsp_pinv_f64): SVD-based, no Gram matrix, singular
% values <= max(size(A))*eps(norm(A)) dropped; min(size) <= 512, max(size) <= 8192; pages of a 3-D A are a batch.
% rcond: smallest kept singular value over the largest, rank: number kept (one entry per page).
  if nargout >= 3
    [P, rcond, rank] = jstsp_mex('pinv_f64', A);
  elseif nargout == 2
    [P, rcond] = jstsp_mex('pinv_f64', A);
  else
    P = jstsp_mex('pinv_f64', A);
  end
end
