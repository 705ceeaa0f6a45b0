function [S_ls, rcond] = ls_estimate_f64(Y, A, B)
% S_ls = pinv(A)*Y*pinv(B) (plot_errorVSsnr.m:83) in float64 on the MI355X (jstsp_ls_f64): nothing is narrowed, and a
% factor of any driver size (up to 512 x 8192) is inverted through its SVD.  A 2-D A or B is shared by the pages of Y.
% rcond = [smallest over the A factors; smallest over the B factors].
  if nargout >= 2
    [S_ls, rcond] = jstsp_mex('ls_f64', Y, A, B);
  else
    S_ls = jstsp_mex('ls_f64', Y, A, B);
  end
end
