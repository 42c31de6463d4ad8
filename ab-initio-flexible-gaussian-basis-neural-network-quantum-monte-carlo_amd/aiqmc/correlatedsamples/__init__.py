"""Correlated sampling between nuclear geometries (AIQMCrelease3/correlatedsamples): the space-warp
transform (corrsamples), its Jacobian (jacobianWeights) and the reweighted energy-difference
estimator with finite-difference forces (estimator)."""
