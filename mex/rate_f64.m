function r = rate_f64(S, Zbar, noise_var)
% log2(real(det(eye(Nr) + 1/Nr*Zbar*Zbar'/(noise_var + nmse)))) of plot_rateVSframelength.m:81, Nr = size(Zbar,1), for a float64
% estimate, computed in float64 on the MI355X (jstsp_rate_f64) as the sum of log2(1 + sigma_k(Zbar)^2/(Nr*(noise_var + nmse)))
% over the singular values of Zbar, with nmse = (norm(S - Zbar)/norm(Zbar))^2 NOT capped.  A third array dimension is the batch:
% every page is scored in ONE call, r has one entry per page.
r = jstsp_mex('rate_f64', S, Zbar, noise_var);
end
