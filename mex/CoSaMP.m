function x = CoSaMP(Phi, y, K)
% The driver's call s_cosamp = CoSaMP(Phi, y, numOfnz) (plot_time_comparisions.m:96).  That function is not vendored:
% this is the published algorithm (Needell & Tropp, Algorithm 1) as include/jstsp.h states it, float64 on the device,
% with the library's defaults of 12 iterations and a relative residual of 1e-6 as the stopping rule.
  x = jstsp_mex('CoSaMP', Phi, y, K);
end
