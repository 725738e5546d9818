"""pyprogressivex — drop-in replacement of the reference's pybind11 module
(/root/reference/src/pyprogressivex/src/bindings.cpp:394-494) on top of libpgx.so (HIP, gfx950).

The five entry points keep the reference's names, argument order, defaults, return layout and error messages;
findPlanes, findSpheres, findLines3D, findCylinders, findCones and findTori (3-D point clouds) and findCircles (2-D point sets) are the same pipeline on model
types the reference does not have; findPrimitives fits planes, spheres, cylinders and cones in one run, and findOrientedPrimitives does so
with inliers that also agree with the points' normals; splitComponents cuts the models of any of these labellings into connected
instances, and instanceExtents bounds each instance on its surface.
"""
from ._api import (PRIMITIVE_CLASSES, estimateNormals, find6DPoses, findCircles, findCones, findCylinders, findFundamentalMatrices, findHomographies, findLines,
                   findLines3D, findOrientedPrimitives, findPlanes, findPrimitives, findSpheres, findTori, findTwoViewMotions, findVanishingPoints, instanceExtents,
                   splitComponents)

__all__ = ["find6DPoses", "findHomographies", "findTwoViewMotions", "findFundamentalMatrices", "findLines",
           "findVanishingPoints", "findPlanes", "findSpheres", "findCircles", "findLines3D", "findCylinders", "estimateNormals",
           "findCones", "findPrimitives", "PRIMITIVE_CLASSES", "findOrientedPrimitives", "findTori", "splitComponents", "instanceExtents"]
