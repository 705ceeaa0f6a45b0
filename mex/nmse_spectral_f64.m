function e = nmse_spectral_f64(S, Zbar)
% min(1, (norm(S - Zbar) / norm(Zbar))^2) with spectral norms (plot_errorVSsnr.m:138-141) for a float64 estimate, computed in
% float64 on the MI355X (jstsp_nmse_spectral_f64): singular values of S - Zbar and of Zbar themselves, nothing narrowed and no
% Gram matrix, so an error 1e-9 of Zbar keeps its digits.  A third array dimension is the batch: every page is scored in ONE
% call, e has one entry per page.  A NaN or Inf in a page gives NaN for that page.
e = jstsp_mex('nmse_spectral_f64', S, Zbar);
end
