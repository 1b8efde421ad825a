# The objects of librsc.so, by source name: <name>.hip kernels with their launchers, <name>.cpp host
# code (compiled as HIP).  Read by the top-level Makefile and by tools/Makefile (A/B libraries).
RSC_HIP_OBJS = kernels mlpnp poseopt sim3opt orbmatch sim3match frameproj kfproj fusekf localproj lastproj kfdb bowvoc triang mpupdate stereo localba
RSC_CPP_OBJS = rsc_api rsc_optim rsc_views rsc_matchers rsc_voc rsc_kfdb rsc_drivers rsc_mappoints rsc_stereo
RSC_OBJS = $(RSC_HIP_OBJS) $(RSC_CPP_OBJS)
