// REFERENCE-BUILD STAND-IN, not OpenCV: see ../core/core.hpp
#pragma once
#include "../core/core.hpp"
